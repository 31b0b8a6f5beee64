/*
 * riichi_mi355x.h — C-ABI of the MI355X-native batched Riichi Mahjong step path.
 *
 * This is the drop-in boundary for the hot path of smly/RiichiEnv:
 *   RiichiEnv.__new__/reset/step/get_observations/done/scores/ranks/mjai_log
 *       (reference: riichienv-python/src/env.rs:82-118, 799-851, 857-872, 741-765,
 *        353-356, 401-404, 673-689, 729-739)
 *   Observation.legal_actions()/mask()          (observation/python.rs:93-111)
 *   HandEvaluator.calc / get_waits / is_tenpai  (hand_evaluator.rs:77-213)
 *   calculate_score                             (score.rs:13-52)
 *
 * One handle = one shard of independent games on one GPU.  All entry points are
 * plain C: opaque handle, caller-allocated arrays, int return code (0 = OK,
 * negative = RMJ_ERR_*).  No torch / C++ types cross this boundary.  A handle is
 * thread-compatible (use one handle per host thread / per GPU).
 *
 * The library has NO CPU fallback: every compute entry point returns
 * RMJ_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef RIICHI_MI355X_H
#define RIICHI_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ constants */
#define RMJ_OK 0
#define RMJ_ERR_ARG (-1)       /* bad argument (ValueError in the reference binding) */
#define RMJ_ERR_NO_DEVICE (-2) /* no usable HIP device / HIP runtime failure at init */
#define RMJ_ERR_HIP (-3)       /* HIP runtime error (see rmj_last_error) */
#define RMJ_ERR_RANGE (-4)     /* index out of range */

#define RMJ_NP 4                /* seats in the 4-player state layout */
#define RMJ_MAX_LEGAL 64        /* max legal actions per seat (reference worst case ~56) */
#define RMJ_ACTION_SPACE_4P 82  /* action.rs:11 */
#define RMJ_ACTION_SPACE_3P 60  /* action.rs:12 */
#define RMJ_MAX_DISCARDS 32
#define RMJ_WALL_4P 136

/* ActionType, action.rs:55-68 */
enum {
    RMJ_DISCARD = 0, RMJ_CHI = 1, RMJ_PON = 2, RMJ_DAIMINKAN = 3, RMJ_RON = 4, RMJ_RIICHI = 5,
    RMJ_TSUMO = 6, RMJ_PASS = 7, RMJ_ANKAN = 8, RMJ_KAKAN = 9, RMJ_KYUSHU = 10, RMJ_KITA = 11
};
/* Phase, action.rs:29-33 */
enum { RMJ_WAIT_ACT = 0, RMJ_WAIT_RESPONSE = 1 };
/* MeldType, types.rs:54-62 */
enum { RMJ_MELD_CHI = 0, RMJ_MELD_PON = 1, RMJ_MELD_DAIMINKAN = 2, RMJ_MELD_ANKAN = 3, RMJ_MELD_KAKAN = 4 };

/* GameRule bits, rule.rs:10-22 (bit i = i-th field) */
#define RMJ_RULE_RON_ON_ANKAN_KOKUSHI 1u
#define RMJ_RULE_KOKUSHI13_DOUBLE 2u
#define RMJ_RULE_SUUANKOU_TANKI_DOUBLE 4u
#define RMJ_RULE_JUNSEI_CHUUREN_DOUBLE 8u
#define RMJ_RULE_DAISUUSHII_DOUBLE 16u
#define RMJ_RULE_PAO_LIABILITY_ONLY 32u
#define RMJ_RULE_SANCHAHO_DRAW 64u
#define RMJ_RULE_KUIKAE_FORBIDDEN 128u
/* Not a GameRule field: seed -> wall as the reference's crates define it (state/wall.rs:36-56: StdRng::seed_from_u64 =
 * PCG32 seed expansion + ChaCha12, SliceRandom::shuffle, salt = next_u64, wall_digest = SHA-256(salt || wall); see
 * rmj_get_wall_digest).  Without the bit the wall of a seed is the build's own counter-based permutation,
 * which costs nothing per round; with it a round start pays one serial Fisher-Yates pass.
 * STATUS OF THE CLAIM: the chain is restated from the published algorithms (rand 0.9 / rand_core 0.9 / chacha20 / sha2); ChaCha, StdRng's
 * construction and SHA-256 are pinned on published vectors, seed_from_u64's PCG32 expansion and the index draws of shuffle on nothing outside
 * this repository - equality of walls and digests with the Rust crates (rand 0.10 in the reference's Cargo.lock) is UNVERIFIED until one real
 * (seed -> wall, salt, digest) vector printed by the reference is pinned in tests/golden/ref_rng_vectors.json (INTEGRATION.md has the Rust
 * program; tests/test_oracle_ref_rng.py and tests/test_gpu_ref_rng.py consume it, and report xfail while it is absent). */
#define RMJ_RULE_REFERENCE_RNG 256u
#define RMJ_RULE_TENHOU (RMJ_RULE_SANCHAHO_DRAW | RMJ_RULE_KUIKAE_FORBIDDEN)          /* rule.rs:31-44 */
#define RMJ_RULE_MJSOUL (1u | 2u | 4u | 8u | 16u | 32u | RMJ_RULE_KUIKAE_FORBIDDEN) /* rule.rs:46-57 */

/*
 * Packed action (u64), used for step() input and for the legal-action lists:
 *   bits  0..7   action type (RMJ_*), 0xFF = "no action from this seat"
 *   bits  8..15  tile (136-id), 0xFF = None
 *   bits 16..23  number of consume tiles (0..4)
 *   bits 24..55  consume tiles c0..c3 (ascending, as Action::new sorts them; action.rs:97-98)
 */
typedef uint64_t rmj_action_t;
#define RMJ_NO_ACTION 0xFFFFFFFFFFFFFFFFull
#define RMJ_TILE_NONE 0xFFu

/* MJAI event record emitted by the device; formatted to the reference's JSON
 * strings (alphabetical keys, state/mod.rs:2094-2148) by rmj_format_event. */
enum {
    RMJ_EV_NONE = 0, RMJ_EV_START_GAME = 1, RMJ_EV_START_KYOKU = 2, RMJ_EV_TSUMO = 3, RMJ_EV_DAHAI = 4,
    RMJ_EV_REACH = 5, RMJ_EV_REACH_ACCEPTED = 6, RMJ_EV_CHI = 7, RMJ_EV_PON = 8, RMJ_EV_DAIMINKAN = 9,
    RMJ_EV_ANKAN = 10, RMJ_EV_KAKAN = 11, RMJ_EV_DORA = 12, RMJ_EV_HORA = 13, RMJ_EV_RYUKYOKU = 14,
    RMJ_EV_END_KYOKU = 15, RMJ_EV_END_GAME = 16, RMJ_EV_KITA = 17,
    RMJ_EV_TEHAI = 18 /* continuation of START_KYOKU: payload[0..25] = 26 hand tiles (2 seats) */
};
/* ryukyoku reasons (state/mod.rs:1846-1968) */
enum {
    RMJ_RK_EXHAUSTIVE = 0, RMJ_RK_NAGASHI = 1, RMJ_RK_KYUSHU = 2, RMJ_RK_SUFUURENTA = 3, RMJ_RK_SUUKANSANSEN = 4,
    RMJ_RK_SUUCHA_RIICHI = 5, RMJ_RK_SANCHAHO = 6, RMJ_RK_ILLEGAL = 7 /* + actor = offender */
};
typedef struct RmjEvent { /* 32 bytes */
    uint8_t type;        /* RMJ_EV_* */
    uint8_t actor;       /* actor / oya (start_kyoku) / offender (illegal ryukyoku) */
    uint8_t target;      /* target / kyoku number (start_kyoku) */
    uint8_t tile;        /* pai / dora_marker */
    uint8_t consumed[4]; /* consumed tiles; start_kyoku: [bakaze, honba, kyotaku_lo, kyotaku_hi] */
    int32_t deltas[4];   /* hora/ryukyoku deltas; start_kyoku: scores */
    uint8_t flags;       /* dahai: tsumogiri; hora: is_tsumo; ryukyoku: reason; n_consumed for melds in bits 4..7 */
    uint8_t n_ura;
    uint8_t ura[5];
    uint8_t pad;
} RmjEvent;

/* ------------------------------------------------------------------ state peek/poke view
 * Mirrors GameState/PlayerState/WallState (state/mod.rs:31-91, state/player.rs:6-39,
 * state/wall.rs:8-19).  Used by tests (the reference's Python setters, env.rs:134-622)
 * and by parity checks: the oracle fills the same struct. */
typedef struct RmjMeldView {
    uint8_t meld_type, n_tiles, tiles[4], opened;
    int8_t from_who;
    int16_t called_tile; /* -1 = None */
} RmjMeldView;

typedef struct RmjPlayerView {
    uint8_t hand_len, hand[14];
    uint8_t n_melds;
    RmjMeldView melds[4];
    uint8_t n_discards, discards[RMJ_MAX_DISCARDS];
    uint32_t discard_from_hand_bits, discard_is_riichi_bits;
    int8_t riichi_declaration_index; /* -1 = None */
    int32_t score, score_delta;
    uint8_t riichi_declared, riichi_stage, double_riichi_declared, missed_agari_riichi, missed_agari_doujun,
        nagashi_eligible, ippatsu_cycle;
    int8_t pao_daisangen, pao_daisuushi; /* liable seat for yaku 37 / 50, -1 = none */
    uint8_t n_forbidden, forbidden[2];
    int16_t riichi_sutehai, last_tedashi; /* -1 = None */
    uint8_t n_kita, kita[4];              /* 3P: kita_tiles (state_3p/player.rs:38) */
} RmjPlayerView;

typedef struct RmjStateView {
    uint8_t wall_len, wall[RMJ_WALL_4P]; /* WallState.tiles (after reverse; draw = pop from end) */
    uint8_t n_dora, dora[5];
    uint8_t rinshan_draw_count, pending_kan_dora_count, drawable_count;
    uint64_t wall_seed, hand_index;
    RmjPlayerView players[RMJ_NP];
    uint8_t current_player, is_done, needs_tsumo, phase, active_mask;
    uint32_t turn_count, riichi_sticks;
    int16_t last_discard_pid, last_discard_tile; /* -1 = None */
    int16_t pending_kan_pid;                     /* -1 = None */
    rmj_action_t pending_kan_action;
    uint8_t oya, honba, kyoku_idx, round_wind, is_rinshan_flag, is_first_turn;
    int16_t riichi_pending_acceptance, drawn_tile; /* -1 = None */
    int16_t last_error_pid;                        /* -1 = no error (quirk Q9) */
} RmjStateView;

/* ------------------------------------------------------------------ configuration */
typedef struct RmjConfig {
    uint32_t n_games;     /* games in this shard */
    uint8_t game_mode;    /* 0..2 = 4p-red-{single,east,half}; 3..5 = 3p (env.rs:93-100) */
    uint8_t skip_mjai_logging;
    uint8_t round_wind;   /* constructor round_wind (env.rs:113) */
    uint8_t reserved0;
    uint32_t rule_bits;   /* RMJ_RULE_* */
    int32_t device;       /* HIP device ordinal */
    uint64_t base_seed;   /* episode seed of game g = splitmix64(base_seed + game_offset + g) unless `seeds` given (consecutive
                             seeds would make game g's k-th hand deal game g+k's first wall, state/wall.rs:38) */
    uint64_t game_offset; /* global index of this shard's first game (multi-GPU sharding by index) */
    const uint64_t* seeds;/* optional [n_games] explicit episode seeds (RiichiEnv(seed=...)) */
    uint32_t event_ring;  /* per-game MJAI event ring capacity (power of two, >= 64) */
    uint32_t reserved1;
} RmjConfig;

typedef struct rmj_env* rmj_handle;

/* ------------------------------------------------------------------ lifecycle */
const char* rmj_version(void);
const char* rmj_last_error(void);
int rmj_device_count(void);
/* RiichiEnv.__new__ (env.rs:82-118): allocates SoA state for n_games, runs the constructor's
 * own _initialize_round (state/mod.rs:165) for every game. */
int rmj_create(const RmjConfig* cfg, rmj_handle* out);
int rmj_destroy(rmj_handle h);

/* RiichiEnv.reset (env.rs:799-851) for the games selected by `select` (NULL = all).
 * Optional per-game arrays (NULL = reference defaults): walls [n][136] in the reference's
 * `wall=` orientation, oya [n], round_wind [n], scores [n][4], honba [n], kyotaku [n]. */
int rmj_reset(rmj_handle h, const uint8_t* select, const uint8_t* walls, const uint8_t* oya, const uint8_t* round_wind,
              const int32_t* scores, const uint8_t* honba, const uint32_t* kyotaku);

/* RiichiEnv.step (env.rs:857-872): actions[n][4] packed, RMJ_NO_ACTION for seats that do not act.
 * Games that are done are left untouched (state/mod.rs:331-333). */
/* RiichiEnv.clone / __copy__ / __deepcopy__ (riichienv-python/src/env.rs:358-372) for the whole batch: a new handle on the same
 * device with the same configuration whose games are in exactly the state of `h`'s - records, walls, published lists / masks /
 * waits / status, event rings, win results (device-to-device copies of the slabs; SURVEY section 5, checkpoint / resume). */
int rmj_clone(rmj_handle h, rmj_handle* out);
/* The complete state of game src_idx[i] of `src` copied into game dst_idx[i] of `dst` (same device, player count and event ring
 * size; dst may be src when the destination games are not among the source games; destination indices distinct): forks for a
 * tree search, a pool of saved positions, refilling slots.  Host index arrays. */
int rmj_copy_games(rmj_handle dst, const uint32_t* dst_idx, rmj_handle src, const uint32_t* src_idx, uint32_t n);
/* Same with the index arrays on the device (a tree search that lives on the GPU): asynchronous on dst's stream; pairs with an index
 * out of range are skipped. */
int rmj_copy_games_device(rmj_handle dst, const uint32_t* d_dst_idx, rmj_handle src, const uint32_t* d_src_idx, uint32_t n);
int rmj_step(rmj_handle h, const rmj_action_t* actions);
/* Same, `actions` is a device pointer (zero-copy from a GPU policy). */
int rmj_step_device(rmj_handle h, const rmj_action_t* d_actions);
/* Device-side uniform-random policy (RandomAgent, src/riichienv/agents/random_agent.py:6-15,
 * keyed per (game, step, seat) — SURVEY §8(c)): choice = mulhi(key32(policy_seed, global_game, step_no, seat), n_legal) (the key: see rmj_step_greedy below)
 * over the ordered legal list.  Runs n_steps batched steps; with auto_reset != 0 a finished game is
 * re-`reset()` (defaults) at the start of the next step instead of stepping.
 * Games are independent, so a rollout of >= 2 steps needs no synchronisation between the steps of different games: it
 * is issued as ONE launch in which every wavefront keeps its four games' records in LDS and steps them n_steps times
 * (kernel k_step4<true>, four games per wavefront); a game whose discard draws claims answers them in the same pass of the
 * wave, so its four games run a step or two ahead of each other inside the launch.  Every game is stepped exactly n_steps times
 * and what the launch leaves behind - records, legal lists up to their counts, masks, waits, status, events - is what n_steps
 * launches of one step leave (entries of the list slab behind a seat's count are unspecified leftovers).  A rollout of >= 32 steps of a batch between one and eight chip-fulls of wavefronts is handed out in pieces instead: a grid
 * that fits the chip once pulls (quad, chunk of up to 64 steps) tickets from per-XCD queues (kernel k_step4_queue; a quad's chunks stay on one XCD, whose L2
 * carries the record from one wavefront to the next), so a batch that is not a whole multiple of the chip's wave slots leaves no
 * half-empty tail (65 536 games: +10 %); RMJ_QUEUE_CHUNK at create sets the chunk length, 0 switches the tickets off.  rmj_set_rollout_streams(h, 1) (or RMJ_STEP_STREAMS=1) makes every step its own launch on the handle's stream - what
 * a policy that is a barrier between steps gets; RMJ_STEP4=1 / 0 in the environment at create selects the earlier
 * schedules (one launch per step and part on up to four streams; one game per wavefront). */
int rmj_step_random(rmj_handle h, uint64_t policy_seed, uint32_t n_steps, int auto_reset);
/* The device policy that PLAYS mahjong (what the consumer of this path runs is a learned policy that wins,
 * riichienv-ml/src/riichienv_ml/trainers/_ppo_worker.py:147-239; the uniform RandomAgent wins once in ~250 rounds): for every
 * seat that is to act, over its ordered legal list, the first entry of the best class
 *   Tsumo / Ron > Kita > Riichi > Ankan > Kakan > Daiminkan > [Pon > Chi, only when (key >> 24) < call_rate_256] >
 *   Discard > Pass > Kyushu kyuhai
 * (Kita before Riichi: the 3P reference offers Kita in the riichi stage and can leave the seat without a legal action),
 * and among the Discard entries (when there are two or more) the one whose removal leaves the concealed hand with the lowest
 * shanten (calculate_shanten / _3p, shanten.rs:228-241 / :454-468, of the remaining tiles with len_div3 = (hand_len - 1) / 3),
 * ties broken by mulhi(key * 0x9E3779B1, #ties) in list order; key = the RandomAgent's 32-bit key of (game, step_no, seat): fmix32 of
 * (lo(gs) ^ (4 * step_no + seat) * 0x9E3779B1) + hi(gs) with gs = splitmix64(policy_seed + global game) - round 6; the RandomAgent takes
 * list entry mulhi(key, n).  Scheduling, auto_reset and outputs exactly like rmj_step_random (same kernels, compiled with this
 * policy in place of the random pick).  Needs the four-games-per-wave kernels (the default; RMJ_STEP4=0 -> RMJ_ERR_ARG). */
int rmj_step_greedy(rmj_handle h, uint64_t policy_seed, uint32_t n_steps, int auto_reset, uint32_t call_rate_256);
/* Fill actions[n][4] with what the device policy would choose for the CURRENT state (no step). */
int rmj_random_actions(rmj_handle h, uint64_t policy_seed, rmj_action_t* actions);
/* Same into a device buffer [n][4], asynchronous on the handle's stream (feeds rmj_step_device without a host trip). */
int rmj_random_actions_device(rmj_handle h, uint64_t policy_seed, rmj_action_t* d_actions);

/* ------------------------------------------------------------------ observations */
int rmj_get_status(rmj_handle h, uint8_t* active_mask, uint8_t* phase, uint8_t* done); /* each [n] */
int rmj_get_legal(rmj_handle h, rmj_action_t* legal /*[n][4][64]*/, uint8_t* counts /*[n][4]*/);
/* The lists a host agent loop reads per step without the [n][4][64] slab (2 KB per game): one row per seat that is to act, in
 * (game, seat) order: index[row] = game * 4 + seat, list = entries[offsets[row] .. offsets[row + 1]) (what Observation.legal_actions()
 * returns for that seat, observation/mod.rs:93-111).  Gathered on the device, copied through pinned staging memory owned by the
 * handle (~110 B per game).  *n_rows / *n_entries: totals of this state; when they exceed cap_rows / cap_entries only the first
 * cap_rows rows / cap_entries entries were written.  offsets has cap_rows + 1 slots. */
int rmj_get_legal_compact(rmj_handle h, uint32_t* index, uint32_t* offsets, rmj_action_t* entries, uint32_t cap_rows, uint32_t cap_entries,
                          uint32_t* n_rows, uint32_t* n_entries);
int rmj_get_mask(rmj_handle h, uint8_t* mask /*[n][4][82]*/);
int rmj_get_waits(rmj_handle h, uint64_t* waits /*[n][4] bit t = tile type t; 0 for seats without an observation (not active, env.rs:870-871) */);
int rmj_get_scores(rmj_handle h, int32_t* scores /*[n][4]*/);
int rmj_get_ranks(rmj_handle h, uint8_t* ranks /*[n][4], 1-based, ties by seat (env.rs:673-689)*/);
int rmj_get_step_counts(rmj_handle h, uint64_t* steps /*[n]*/);
int rmj_total_steps(rmj_handle h, uint64_t* total);
/* state.wall.salt / state.wall.wall_digest (riichienv-core/src/state/wall.rs:15-16, 48-55; state_3p/wall.rs:52-53, 91-99): the salt as 16
 * hex digits and SHA-256(salt || wall before the reversal) as 64, NUL-terminated.  Set by a seeded shuffle under RMJ_RULE_REFERENCE_RNG, left
 * alone by an injected wall (load_wall), cleared by a start_kyoku event (event_handler.rs:81-82); empty strings otherwise.  The digest is
 * computed on the device when asked for (salt and wall are state; the hash is a function of them). */
int rmj_get_wall_digest(rmj_handle h, uint32_t game, char* salt /*[17]*/, char* digest /*[65]*/);
int rmj_get_wall_digests(rmj_handle h, uint32_t first, uint32_t n, char* salts /*[n][17]*/, char* digests /*[n][65]*/);
int rmj_peek_state(rmj_handle h, uint32_t game, RmjStateView* out);
/* The observation outputs of ONE game (get_observations of its acting seats, env.rs:741-765): legal [4][64] + counts [4],
 * mask [4][82], waits [4], status = active_mask | phase << 8 | is_done << 16.  For sampled checks of large batches. */
int rmj_peek_outputs(rmj_handle h, uint32_t game, rmj_action_t* legal, uint8_t* counts, uint8_t* mask, uint64_t* waits,
                     uint32_t* status);
int rmj_poke_state(rmj_handle h, uint32_t game, const RmjStateView* in); /* recomputes legal actions */

/* RiichiEnv.win_results (env.rs:606-607; state/mod.rs:60, 863, 1107, 1729): the WinResult of every seat that won the
 * current round, with its pao payer.  The reference clears the map whenever a round is initialised, so it is non-empty
 * only while the game is over (the round that ended it was won).  out[4] is indexed by seat; *seat_mask tells which
 * entries are set. */
typedef struct RmjWinResult { /* WinResult, types.rs:282-293 */
    uint8_t is_win, yakuman, has_win_shape, n_yaku;
    uint8_t yaku[20];
    uint32_t han, fu, ron_agari, tsumo_agari_oya, tsumo_agari_ko;
    int8_t pao_payer; /* -1 = None */
    uint8_t pad[3];
} RmjWinResult;
int rmj_get_win_results(rmj_handle h, uint32_t game, RmjWinResult* out /*[4]*/, uint8_t* seat_mask);

/* MJAI events: records of the CURRENT game's log per slot (len(mjai_log): a reset / auto-reset starts it again, state/mod.rs:171-187),
 * and a window of them (`first` counts from the current game's first record). */
int rmj_get_event_counts(rmj_handle h, uint32_t* counts /*[n]*/);
int rmj_get_events(rmj_handle h, uint32_t game, uint32_t first, uint32_t max_events, RmjEvent* out, uint32_t* n_out);
/* Formats one event (START_KYOKU consumes the 2 TEHAI continuation records that follow it; returns
 * the number of records consumed, or <0).  seat = -1 -> full log string, 0..3 -> per-seat masked view. */
int rmj_format_event(const RmjEvent* ev, uint32_t n_avail, int seat, char* buf, uint32_t cap);
/* The logs of MANY games at once (RiichiEnv.mjai_log / the per-seat logs of every env, riichienv-python/src/env.rs:729-739,
 * state/mod.rs:2094-2148).
 * Every game SLOT writes one record stream: its position (the number of records the slot has emitted since rmj_create) never goes
 * back - a restart by auto-reset / rmj_reset / a start_game event only moves the position at which the current game's log begins
 * (rmj_get_log_positions: base) - and record i sits in ring slot i & (ring - 1) whichever game wrote it.  Cursors are such positions,
 * so a cursor stays valid across restarts and a window may hold the end of one game and the start of the next.
 * rmj_drain_events: the records every slot wrote since cursor[g] (0 = from the start of the stream), gathered on the device into
 * one dense buffer and copied down once: slot g's records are out[offsets[g] .. offsets[g + 1]) (offsets has n + 1 slots),
 * cursor[g] becomes the slot's position.  A slot whose ring was lapped since its cursor has lost its oldest records: the window
 * then starts at the oldest one still there and the loss is added to RmjEventViews.lost[g] - by the call that hands the window
 * over, not by a failed call, and not under RMJ_DRAIN_PEEK (cursors are then input only: a look at the rings).  When more than
 * cap_events records are waiting nothing is drained, *n_events holds the number, the result is RMJ_ERR_RANGE.
 * rmj_format_events: the strings of such a buffer, formatted by a pool of host threads: game g's log - its events' strings, each
 * followed by '\n' - is buf[text_offsets[g] .. text_offsets[g + 1]); *needed = bytes of all logs; RMJ_ERR_RANGE (nothing written) when
 * cap is smaller.  seat as in rmj_format_event.
 * rmj_drain_format: both in one call through pinned staging owned by the handle (no intermediate copy); ms, when given, receives the
 * milliseconds of the device gather, the copy to the host and the formatting.  A size call (buf = NULL: RMJ_ERR_RANGE, *needed set)
 * keeps what it gathered; the call that follows with the same cursors and seat only formats (the drain is "as of the size call").
 * rmj_get_log_positions: per slot, where the current game's log begins (base) and the stream position (pos); either may be NULL. */
#define RMJ_DRAIN_PEEK 1u
int rmj_get_log_positions(rmj_handle h, uint32_t* base /*[n]*/, uint32_t* pos /*[n]*/);
int rmj_drain_events(rmj_handle h, uint32_t* cursor /*[n] in/out*/, RmjEvent* out, uint32_t cap_events, uint32_t* offsets /*[n + 1]*/, uint32_t* n_events,
                     uint32_t flags);
int rmj_format_events(const RmjEvent* ev, const uint32_t* offsets, uint32_t n_games, int seat, char* buf, uint64_t cap, uint64_t* text_offsets /*[n + 1]*/,
                      uint64_t* needed);
int rmj_drain_format(rmj_handle h, uint32_t* cursor /*[n] in/out*/, int seat, char* buf, uint64_t cap, uint64_t* text_offsets /*[n + 1]*/, uint64_t* needed,
                     uint32_t* n_events, double* ms /*[3] or NULL*/, uint32_t flags);
/* Device views of the event stream for a consumer on the same GPU: slot g's record i (a stream position, i < count) sits at
 * events[g * ring + (i & (ring - 1))] while count - i <= ring; count = *(const uint32_t*)((const char*)ev_count + g * ev_count_stride);
 * the current game's log begins at position *(const uint32_t*)((const char*)ev_base + g * ev_count_stride). */
typedef struct RmjEventViews {
    uint32_t n_games, ring;
    const RmjEvent* events;      /* [n][ring] */
    const uint32_t* ev_count;    /* first game's record count; the others follow at ev_count_stride bytes */
    uint32_t ev_count_stride, reserved;
    const uint32_t* lost;        /* [n] records lost to a late drain, cumulative */
    const uint32_t* ev_base;     /* first slot's log base; the others follow at ev_count_stride bytes */
} RmjEventViews;
int rmj_event_views(rmj_handle h, RmjEventViews* out);
int rmj_get_events_lost(rmj_handle h, uint32_t* lost /*[n]*/); /* host copy of RmjEventViews.lost */
/* MJAI text formatted on the device: the same bytes and offsets as rmj_drain_format / rmj_format_events (the host formatter), written
 * by a HIP formatter, every game's log at text[text_offsets[g] .. text_offsets[g + 1]) (its events' strings, each followed by '\n').
 * rmj_drain_text: the drain contract above - cursors are stream positions and survive restarts, a lapped window starts at the oldest
 * record still held and the loss is booked in RmjEventViews.lost by the call that hands the text over, RMJ_DRAIN_PEEK moves nothing,
 * cursors advance exactly as rmj_drain_format advances them - with the records read in place from the rings (no record copy).
 * rmj_format_events_device: the device analogue of rmj_format_events, over caller records already on the device (game g's records
 * d_ev[d_offsets[g] .. d_offsets[g + 1])).
 * The text and its offsets live in buffers owned by the handle (not its scratch): the view stays valid until the next rmj_drain_text /
 * rmj_format_events_device on the handle, or rmj_destroy.  Without RMJ_TEXT_ON_DEVICE the view points at pinned host memory (the device
 * text plus ONE copy); with it, at device memory.  Both calls synchronise the handle's stream before they return: the text is complete
 * and a consumer on any stream may read the view at once.  ms: device format, copy to the host (0 on device delivery), total.
 * Either call ends what a size call of rmj_drain_format staged (as rmj_drain_events does). */
typedef struct RmjTextView {
    const char* text;             /* [bytes]: game g's log is text[text_offsets[g] .. text_offsets[g + 1]) */
    const uint64_t* text_offsets; /* [n_games + 1] */
    uint64_t bytes;
    uint32_t n_games, n_events;
    double ms[3]; /* device format, copy to host (0 on device delivery), total */
} RmjTextView;
#define RMJ_TEXT_ON_DEVICE 2u /* with RMJ_DRAIN_PEEK (1u): the view's pointers are device pointers */
int rmj_drain_text(rmj_handle h, uint32_t* cursor /*[n] in/out*/, int seat, uint32_t flags, RmjTextView* out);
int rmj_format_events_device(rmj_handle h, const RmjEvent* d_ev, const uint32_t* d_offsets /*[n_games + 1]*/, uint32_t n_games, int seat,
                             uint32_t flags, RmjTextView* out);

/* ------------------------------------------------------------------ batched hand math (kernel gate) */
typedef struct RmjHandCase {
    uint8_t n_tiles, tiles[14];
    uint8_t n_melds;
    RmjMeldView melds[4];
    uint8_t win_tile;
    uint8_t n_dora, dora[5], n_ura, ura[5];
    /* Conditions, types.rs:193-210 */
    uint8_t tsumo, riichi, double_riichi, ippatsu, haitei, houtei, rinshan, chankan, tsumo_first_turn;
    uint8_t player_wind, round_wind, kita_count, is_sanma;
    uint32_t honba;
} RmjHandCase;
typedef struct RmjHandResult { /* WinResult, types.rs:282-293 */
    uint8_t is_win, yakuman, has_win_shape, n_yaku;
    uint8_t yaku[20];
    uint32_t han, fu, ron_agari, tsumo_agari_oya, tsumo_agari_ko;
    uint64_t waits; /* HandEvaluator.get_waits of the tiles/melds (13-tile hands), bit per type */
    uint8_t is_tenpai, is_agari, pad[6];
} RmjHandResult;
int rmj_eval_hands(int device, const RmjHandCase* cases, uint32_t n, RmjHandResult* out);
/* agari.rs:65-73 / hand_evaluator.rs:178-213 over raw 34-histograms */
int rmj_agari_counts(int device, const uint8_t* counts /*[n][34]*/, uint32_t n, uint8_t* is_agari, uint8_t* is_tenpai,
                     uint64_t* waits);
/* score.rs:13-52 */
int rmj_calculate_score(int device, const uint8_t* han, const uint8_t* fu, const uint8_t* is_oya, const uint8_t* is_tsumo,
                        const uint32_t* honba, const uint8_t* num_players, uint32_t n, uint32_t* out /*[n][4] total,ron,oya,ko*/);

/* Observation.encode() (observation/python.rs:457-806, docs/FEATURE_ENCODING.md): 74 x 34 f32, channel-major, for
 * every seat of every game: out[n][4][74][34].  only_active != 0 -> seats that are not to act get zeros. */
#define RMJ_ENC_CHANNELS 74
#define RMJ_ENC_WIDTH_4P 34
#define RMJ_ENC_WIDTH_3P 27 /* 3P: out[n][4][74][27], compact tile index (observation_3p/helpers.rs:3-15) */
/* only_active: 0 = every seat, 1 = acting seats (rows of the others are zeroed), 2 = acting seats, rows of the others
 * are left untouched (no HBM traffic for them; meant for resident device buffers) */
int rmj_encode(rmj_handle h, int only_active, float* out);
/* Row stride of the outputs of the BASE encoder (this function, rmj_encode_device, rmj_encode_compact_device, rmj_step_random_encode,
 * rmj_step_ids_encode_device): every (game, seat) row of 74 x W floats starts `floats` floats after the previous one (out[n][4][floats],
 * compact: out[capacity][floats]); 0 = dense (74 x W, the default).  Rows padded to a multiple of 256 B - 2 048 floats in 3P, 2 560 in
 * 4P - are written at 1.3-1.4 x the rate of the unaligned dense rows (the acting seats' rows are one row in four of the tensor; DESIGN.md
 * section 11.7); the pad floats are never written.  `floats` must be even and >= 74 x W. */
int rmj_set_encode_row_stride(rmj_handle h, uint32_t floats);
int rmj_encode_device(rmj_handle h, int only_active, float* d_out); /* device pointer, asynchronous on the handle's stream */
/* Device-policy rollout WITH feature output (BASELINE configs[4]): n_steps x (one step of every game, then encode() of the
 * seats that are to act into the resident tensor d_out).  Same results as calling rmj_step_random(h, seed, 1, auto_reset)
 * and rmj_encode_device(h, only_active, d_out) n_steps times; issued like rmj_step_random as up to four parts of the batch on
 * as many HIP streams, each part running step, encode, step, encode ... in order. */
int rmj_step_random_encode(rmj_handle h, uint64_t policy_seed, uint32_t n_steps, int auto_reset, int only_active, float* d_out);
/* The batch a trainer stacks from the reference's `{pid: obs.encode() for pid, obs in env.step(...).items()}`
 * (riichienv-python/src/env.rs:857-872, observation/python.rs encode): the Observation.encode() tensors of the ACTING seats
 * only, one after the other in (game, seat) order.  d_out: [capacity][74][34 | 27] f32, d_index: [capacity] i32 = game * 4 + seat
 * of every row, *d_count (device u32): the number of observations of this state (finished games have none); when it exceeds
 * `capacity` only the first `capacity` rows were written.  Dense rows instead of 1 row in 4 of the [n_games][4] tensor:
 * the same bytes leave at 1.6x the rate.  Asynchronous on the handle's stream. */
int rmj_encode_compact_device(rmj_handle h, float* d_out, int32_t* d_index, uint32_t capacity, uint32_t* d_count);
/* rmj_step_random(h, seed, 1, auto_reset) + rmj_encode_compact_device n_steps times (one stream): BASELINE configs[4]. */
int rmj_step_random_encode_compact(rmj_handle h, uint64_t policy_seed, uint32_t n_steps, int auto_reset, float* d_out, int32_t* d_index,
                                   uint32_t capacity, uint32_t* d_count);

/* Observation.encode_extended (observation/python.rs:1271-1296): 215 channels = encode() + discard decay (4), shanten
 * efficiency (16), ankan (4), fuuro (80), action availability (11), discard candidates (5), pass context (3), last
 * tedashis (9), riichi sutehais (9); observation/encode.rs:293-585, observation_3p/encode.rs:315-615.
 * out[n][4][215][34] (3P: [n][4][215][27], seat 3 zero). */
#define RMJ_ENC_EXT_CHANNELS 215
int rmj_encode_extended(rmj_handle h, int only_active, float* out);
int rmj_encode_extended_device(rmj_handle h, int only_active, float* d_out); /* device pointer, asynchronous on the handle's stream */

/* Observation batches for a trainer: the ACTING seats' tensors of one feature set, written as the policy consumes them.
 *   RMJ_FEATURES_BASE             Observation.encode() (observation/python.rs:457-806): 74 x W.
 *   RMJ_FEATURES_DISCARD_SHANTEN  riichienv-ml feat_v2.DiscardHistoryShantenEncoder (configs/4p/ppo_v2.yml, in_channels 94): encode()
 *                                 (rows 0..73), then encode_discard_history_decay() (74..77, decay rate 0.2) and encode_shanten_efficiency()
 *                                 broadcast over the columns (78..93) - rows 74..93 of encode_extended().  94 x 34, 4P only: the
 *                                 reference's 3P observation has 3 decay rows and a (3, 4) efficiency block that feat_v2 cannot reshape.
 *   RMJ_FEATURES_EXTENDED         Observation.encode_extended() (riichienv-ml feat_v3.ExtendedEncoder): 215 x W, the rows of
 *                                 rmj_encode_extended_device.
 * compact = 0: out[n][4][row_stride], the rows of the acting seats (the others untouched, like only_active = 2).
 * compact = 1: out[capacity][row_stride] holding the acting seats one after the other in (game, seat) order, index[slot] = game * 4 + seat,
 *              *count (device u32) = the number of acting seats of this state; when it exceeds `capacity` only the first `capacity`
 *              rows (and index entries) were written - what rmj_encode_compact_device does for encode().
 * row_stride: floats from one row to the next, even and >= C x W; 0 = C x W (dense rows; 215 x 27 is odd: such rows may start 4-byte
 * aligned).  The pad floats are never written.  All pointers are device pointers. */
#define RMJ_FEATURES_BASE 0            /* Observation.encode(): 74 x W */
#define RMJ_FEATURES_DISCARD_SHANTEN 1 /* riichienv-ml feat_v2: encode() + decay (4) + shanten efficiency (16, broadcast); 94 x 34, 4P only */
#define RMJ_FEATURES_EXTENDED 2        /* Observation.encode_extended(): 215 x W */
#define RMJ_FEATURES_DISCARD_SHANTEN_CHANNELS 94
typedef struct RmjObsBatch {
    int32_t features;     /* RMJ_FEATURES_* */
    int32_t compact;      /* 0: out[n][4][row_stride], acting rows only; 1: out[capacity][row_stride] + index + count */
    uint32_t row_stride;  /* floats; 0 = C x W */
    uint32_t capacity;    /* compact only */
    float* d_out;
    int32_t* d_index;     /* compact only: [capacity] game * 4 + seat */
    uint32_t* d_count;    /* compact only: device u32 */
} RmjObsBatch;
/* The batch of the current state, asynchronous on the handle's stream.  RMJ_ERR_ARG for DISCARD_SHANTEN on a 3P handle, an unknown
 * feature set, a bad row stride or a missing pointer (d_index / d_count are needed with compact = 1 only). */
int rmj_encode_batch_device(rmj_handle h, const RmjObsBatch* b);
/* The same with host pointers (d_out / d_index / d_count of `b` point to host memory): staged on the device, returns when the rows are
 * there.  Dense: rows of seats that do not act keep what `d_out` held. */
int rmj_encode_batch(rmj_handle h, const RmjObsBatch* b);
/* rmj_step_ids_device(h, d_action_ids, auto_reset) + rmj_encode_batch_device(h, b): the trainer loop's iteration (riichienv-ml
 * trainers/_ppo_worker.py:151-239: step, then the encoder of the returned observations) for every feature set.  The same state and rows
 * as the two calls; separate launches on the handle's stream, no host synchronisation between them. */
int rmj_step_ids_encode_batch_device(rmj_handle h, const int32_t* d_action_ids, int auto_reset, const RmjObsBatch* b);
/* rmj_sample_ids_device(h, d_logits, stride, seed, d_ids) + rmj_step_ids_device(h, d_ids, auto_reset) + rmj_encode_batch_device(h, b):
 * the whole environment side of a trainer iteration between two policy forward passes.  d_ids [n][4] receives the drawn ids. */
int rmj_step_sample_encode_batch_device(rmj_handle h, const float* d_logits, uint32_t stride, uint64_t seed, int auto_reset,
                                        int32_t* d_ids, const RmjObsBatch* b);

/* Hidden-hand targets: what the observation hides from a seat - the concealed tiles, shanten number, waits and flags of its three
 * opponents - read from the complete state on the device (auxiliary heads for opponent tenpai / waits / hand; the input of an oracle
 * or perfect-information critic).  For the pair (game g, hero seat a) opponent r = 0, 1, 2 is seat (a + 1 + r) mod NP: shimocha,
 * toimen, kamicha; in 3P r = 2 is absent (every field zero, flags 0), and so is every opponent of a row whose index names no
 * (game, seat < NP) of the handle.
 *   d_opp_hand    [rows][3][34] u8  concealed tiles by tile type (red fives count as fives; 34 columns in 3P too)
 *   d_opp_shanten [rows][3] i8      calculate_shanten / calculate_shanten_3p (shanten.rs:244-261 / :470-484) of that histogram with
 *                                   total / 3 groups: rmj_shanten of the same row (-1 = complete; chiitoi and kokushi with four groups)
 *   d_opp_waits   [rows][3] u64     bit t: HandEvaluator(hand, melds).get_waits() holds type t (hand_evaluator.rs:196-213) - empty
 *                                   unless concealed + 3 x melds = 13; a type already held four times is skipped
 *   d_opp_flags   [rows][3] u8      RMJ_HIDDEN_* bits, n_melds in bits 4..6 */
#define RMJ_HIDDEN_PRESENT 1u  /* the opponent exists */
#define RMJ_HIDDEN_TENPAI 2u   /* waits != 0 */
#define RMJ_HIDDEN_RIICHI 4u   /* riichi_declared */
#define RMJ_HIDDEN_FURITEN 8u  /* the waits meet a type of the seat's discards, or missed_agari_doujun, or missed_agari_riichi */
#define RMJ_HIDDEN_MELDS_SHIFT 4
typedef struct RmjHiddenOut {
    uint8_t* d_opp_hand;
    int8_t* d_opp_shanten;
    uint64_t* d_opp_waits;
    uint8_t* d_opp_flags;
} RmjHiddenOut;
/* The rows of d_index [rows] i32 = game * 4 + seat - what rmj_encode_compact_device and rmj_get_legal_compact hand out, or any other
 * (game, seat), acting or not - into the caller's device arrays.  d_count (device u32, may be NULL): rows at or behind
 * min(rows, *d_count) are left untouched, so the count of a compact batch can stay on the device.  Only reads the state (no cache is
 * written back).  Asynchronous on the handle's stream.  RMJ_ERR_ARG for a null handle / descriptor, or null arrays with rows > 0. */
int rmj_hidden_targets_device(rmj_handle h, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, const RmjHiddenOut* out);
/* The same with host pointers (index and the four arrays of `out`): staged on the device, returns when the rows are there. */
int rmj_hidden_targets(rmj_handle h, const int32_t* index, uint32_t rows, const RmjHiddenOut* out);

/* Deal-in danger targets: for the pair (game g, hero seat a), every opponent r (seat (a + 1 + r) mod NP, as above) and every tile kind k,
 * the points that opponent would win by ron if the hero discarded a tile of that kind now - the label of a danger head, a folding
 * policy or a search leaf.  A wait of rmj_hidden_targets_device that is furiten, or whose hand has a win shape and no yaku, costs
 * nothing; a live one costs what the hand evaluator says.  Kinds 0..33: tile type k as its non-red id 4 k + 1; kinds 34, 35, 36: ids
 * 16, 52, 88 - copy 0 of the fives, the red ones where the mode has them (the mode is not consulted).
 *   d_danger [rows][3][37] i32  0 unless seat s holds concealed + 3 x melds = 13, the type of k is among its waits, neither that type
 *   nor any other wait of s is among s's own discards, neither missed_agari flag is set, and the hand wins (a yaku other than dora, or
 *   a yakuman); then ron_agari of the evaluation under the seat's riichi / double riichi / ippatsu, houtei when drawable_count == 0 and
 *   not is_rinshan, the seat's and the round's wind, the dora indicators revealed now, kita_count = n_kita in 3P and the table's honba,
 *   with a double yakuman whose rule bit is off counted once: the ron branch of the claim generation, then the winner's part of the ron
 *   settlement.  RMJ_DANGER_URA: a seat in riichi also counts its ura indicators, read from the wall (the settlement's indices).
 * Not what the settlement moves in these respects: riichi sticks on the table are not part of the value (the winner takes them, the
 * discarder does not pay them); a pao split is not applied (the value is the winner's gain; with a liable third seat the discarder
 * pays less); of several simultaneous winners only the nearest takes honba, here every opponent is valued as the only winner; the
 * sanchaho draw is ignored; a kan-dora indicator pending at the moment of the row (pending_kan_dora_count > 0) is revealed with the
 * discard itself and is not counted.
 * Index, d_count and the absent rows as in rmj_hidden_targets_device; only reads the state.  Asynchronous on the handle's stream.
 * RMJ_ERR_ARG for a null handle / descriptor, an unknown flag, or null arrays with rows > 0. */
#define RMJ_DANGER_URA 1u
#define RMJ_DANGER_KINDS 37
typedef struct RmjDangerOut {
    int32_t* d_danger;   /* [rows][3][37] */
} RmjDangerOut;
int rmj_danger_targets_device(rmj_handle h, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, uint32_t flags, const RmjDangerOut* out);
/* The same with host pointers (index and the array of `out`): staged on the device, returns when the rows are there. */
int rmj_danger_targets(rmj_handle h, const int32_t* index, uint32_t rows, uint32_t flags, const RmjDangerOut* out);

/* Discard efficiency table: for a hand, the shanten after every discard, the draws that then lower it and how many of them are live -
 * the attack value of each of the 34 tile types, next to the defence cost rmj_danger_targets_device gives; what rmj_best_ukeire and
 * rmj_effective_tiles fold to one number.  For a hand histogram c[34] of n tiles and a visible histogram v[34]:
 *   valid types   all 34 in 4P; type 0 and types 8..33 in 3P
 *   sh(x)         rmj_shanten of x (calculate_shanten / calculate_shanten_3p with tiles / 3 groups)
 *   for a hand x of 3k+1 tiles:  A(x) = { t valid : x[t] < 4 and sh(x + t) < sh(x) },  accept(x) = |A(x)|,
 *                 ukeire(x) = sum over t in A of max(0, max(0, 4 - v[t]) - x[t]),  mask(x) = the bits of A
 *   column t < 34 if n % 3 == 2 and c[t] > 0: with x = c - e_t, shanten[t] = sh(x), accept[t], ukeire[t], mask[t] - discards that raise
 *                 the shanten too; otherwise shanten[t] = RMJ_DTAB_NONE and the rest 0.  A held 2m..8m of a raw 3P histogram gets its
 *                 column like any other type.
 *   column 34     the hand itself: shanten[34] = sh(c).  n % 3 == 1: accept and mask of c.  n % 3 == 2: accept[34] and ukeire[34]
 *                 are, separately, the maxima over the t with shanten[t] <= shanten[34] (rmj_effective_tiles, rmj_best_ukeire),
 *                 mask[34] = 0.  n % 3 == 0: the shanten only.
 *                 ukeire[34] of a 3n+1 hand is rmj_best_ukeire of it as well, NOT ukeire(c): calculate_best_ukeire walks the discards
 *                 of a hand of any size - the maximum of ukeire(c - e_d) over the held d with sh(c - e_d) <= sh(c), the 3n hands
 *                 judged with (n - 1) / 3 groups.  So column 34 is, for every hand, what rmj_shanten, rmj_effective_tiles and
 *                 rmj_best_ukeire answer and what channels 78..80 of the extended features carry (x 8, x 34 or 27, x 80).
 *   d_shanten [rows][35] i8,  d_accept [rows][35] u8,  d_ukeire [rows][35] u8 (at most 136),  d_mask [rows][35] u64 (may be NULL)
 * An absent row (index out of range, seat >= the number of players) has every shanten RMJ_DTAB_NONE and the rest 0.
 * The row of (game g, seat a): c = the seat's concealed tiles by type, v = the histogram the efficiency channels of the extended
 * features count - every seat's discards, every seat's meld tiles (4 for kans) and the revealed dora indicators.  By tile type: red
 * fives are fives.
 * Index, d_count and the untouched tail as in rmj_hidden_targets_device; only reads the state (no cache is written back).  Asynchronous
 * on the handle's stream.  flags must be 0.  RMJ_ERR_ARG for a null handle / descriptor, a flag, or null arrays with rows > 0. */
#define RMJ_DTAB_NONE 127
#define RMJ_DTAB_COLS 35
typedef struct RmjDiscardTableOut {
    int8_t* d_shanten;    /* [rows][35] */
    uint8_t* d_accept;    /* [rows][35] */
    uint8_t* d_ukeire;    /* [rows][35] */
    uint64_t* d_mask;     /* [rows][35], may be NULL */
} RmjDiscardTableOut;
int rmj_discard_table_device(rmj_handle h, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, uint32_t flags, const RmjDiscardTableOut* out);
/* The same with host pointers (index and the arrays of `out`): staged on the device, returns when the rows are there. */
int rmj_discard_table(rmj_handle h, const int32_t* index, uint32_t rows, uint32_t flags, const RmjDiscardTableOut* out);
/* The table of raw histograms on the host, like rmj_best_ukeire: counts [n][34] u8, visible [n][34] u8 or NULL (nothing visible), host
 * arrays in `out` ([n][35]; the mask may be NULL).  A hand of more than 14 tiles, or a count above 4, gives an absent row. */
int rmj_discard_table_hands(int device, const uint8_t* counts, const uint8_t* visible, uint32_t n, int sanma, const RmjDiscardTableOut* out);

/* Determinize: re-deal, in place, what seat a of game g cannot see - the concealed hands of its opponents and the part of the wall that can
 * still be drawn or revealed - so that the game becomes a position the seat could not tell from the one it was; lists, masks, waits and
 * status are republished and every call steps the game on (forks of rmj_copy_games_device become sampled worlds: PIMC, determinized
 * search, value targets).  The pool in canonical order, in terms of RmjStateView: for r = 0, 1, 2 with r + 1 < NP and bit r of the row's
 * `hold` byte clear, players[(a + 1 + r) mod NP].hand[0 .. hand_len); then wall[j], j ascending, except the revealed dora indicators
 * (j + rinshan_draw_count = D + 2 k, k < n_dora; D = 4, in 3P 8).  The permutation:
 *   mix(z):  z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31  (mod 2^64)
 *   base  = mix(seed + global game)   (RmjConfig.game_offset + g, as the device policies count games)
 *   key_i = mix(base + (a * 256 + i) * 0x9E3779B97F4A7C15),  i = canonical index;  perm = the indices sorted by (key_i, i)
 *   the new tile at canonical position r is the old tile at canonical position perm[r]
 * Then re-dealt hands are sorted (a re-dealt current player that holds a drawn tile keeps its last slot last; drawn_tile names the tile now
 * there), in RMJ_WAIT_RESPONSE the claims of every seat but the discarder are rebuilt from the new hands (active_mask follows; seat a's own
 * list, mask row and waits stay byte for byte), player flags stay, claim lists kept from before an accepted call are dropped as
 * rmj_poke_state drops them, and salt / wall digest go on answering what they answered.  The event ring is NOT rewritten: the log of a
 * determinized game no longer describes the opponents' tiles.  The sample is uniform over tile placements, not over worlds consistent
 * with a riichi declaration (bits 4..6 of the status) - unless the repair below is asked for.
 *
 * RMJ_DETF_RIICHI_TENPAI (rmj_determinize_ex_device / rmj_determinize_ex): re-dealt riichi hands are walked to tenpai.  The repair runs
 * after the permutation has been applied and before the re-dealt hands are sorted, on the pool and the canonical indices above.
 *   Partners:  Q = the canonical indices whose location is not a hand slot of a seat that has declared riichi - the wall entries of the
 *     pool and the hands of the re-dealt opponents that are not in riichi.
 *   Seats:  r = 0, 1, 2 in that order, with r + 1 < NP and bit r of `hold` clear; seat s = (a + 1 + r) mod NP is repaired if it has declared
 *     riichi and hand_len = n with n mod 3 = 1.  Any other riichi seat is left to its NOTEN bit.
 *   The walk of one seat:  cur = shanten(hand) - calculate_shanten, in 3P calculate_shanten_3p, with len_div3 = n / 3 (rmj_shanten).
 *     For k = 0 .. 11 while cur > 0:  over hand slots i < n (tile x, type d = x >> 2) and partners j in Q (tile y, type t = y >> 2) with
 *     d != t let v = shanten(hand - d + t).  want = cur - 1 if any pair reaches it, otherwise want = cur (a sideways step); if no pair has
 *     v == want the walk stops.  Among the pairs with v == want the one with the smallest (key, i, j) is taken,
 *       key = mix(base + (1024 + ((((a * 4 + r) * 16 + k) * 16 + i) * 256 + j)) * 0x9E3779B97F4A7C15)      (rmj_determinize_swap_key)
 *     with mix and base as for the permutation (the offset 1024 keeps these keys off the permutation's); x and y are exchanged in place,
 *     nothing is sorted in between, and cur = want.
 * Then everything goes on as without the flag: the re-dealt hands are sorted (a drawn-tile slot stays last), the waits cache is cleared,
 * the claims are rebuilt, the outputs are published and the NOTEN bits are computed from the final hands (waits == 0).  RMJ_DET_SWAPPED
 * is set in the status of a row in whose world at least one exchange was made.  Choosing over concrete (slot, partner) pairs weights a
 * pair of types by its multiplicities; the sideways steps are what lets the walk leave a hand no single exchange improves.
 * What this distribution is: the nearest tenpai hand by fewest exchanges from a uniform deal, with seeded ties.  It is NOT a posterior.
 * Out of scope: furiten consistency with the seat's own discards or with passed tiles; weighting by discards or calls; rewriting the
 * event ring; riichi seats with n mod 3 = 2 (a riichi seat holding its drawn tile).
 * d_status [rows] u8 (may be NULL): */
#define RMJ_DET_OK 0u
#define RMJ_DET_NOT_ACTING 1u    /* index out of range (negative too), seat >= NP, game done, or seat not in active_mask: game untouched */
#define RMJ_DET_CHANKAN 2u       /* a robbed kan / kita is pending (pending_kan_pid set): its claims cannot be rebuilt; game untouched */
#define RMJ_DET_DUPLICATE 3u     /* another row of the call that could be carried out names the same game and has a lower row number: of such rows exactly the lowest is carried out */
#define RMJ_DET_RIICHI_NOTEN 16u /* << r: opponent r was re-dealt, has declared riichi and its 13 new tiles are not tenpai (with RMJ_DET_OK in the low bits) */
#define RMJ_DET_SWAPPED 128u     /* RMJ_DETF_RIICHI_TENPAI made at least one exchange in the row's world (with RMJ_DET_OK in the low bits) */
#define RMJ_DETF_RIICHI_TENPAI 1u /* flags of rmj_determinize_ex*: walk the re-dealt riichi hands to tenpai (above) */
typedef struct RmjDeterminize {
    uint64_t seed;
    const uint8_t* d_hold;   /* [rows] or NULL: bit r set = opponent r (seat (a + 1 + r) mod NP) keeps its concealed hand */
    uint8_t* d_status;       /* [rows] or NULL */
} RmjDeterminize;
/* The rows of d_index [rows] i32 = game * 4 + seat (as rmj_encode_compact_device and rmj_get_legal_compact hand them out); d_count (device
 * u32, may be NULL): rows at or behind min(rows, *d_count) are left untouched, their status too.  Asynchronous on the handle's stream (the
 * first call of a handle allocates its claim words).  RMJ_ERR_ARG for a null handle / descriptor / index with rows > 0. */
int rmj_determinize_device(rmj_handle h, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, const RmjDeterminize* p);
/* The same with host pointers (index, d_hold, d_status): staged on the device, returns when done.  Two rows that name one game are
 * refused with RMJ_ERR_ARG before anything is touched. */
int rmj_determinize(rmj_handle h, const int32_t* index, uint32_t rows, const RmjDeterminize* p);
/* perm [m] of the permutation above for (seed, global game, seat, m <= 256), from the code the kernel runs; host only, needs no GPU. */
int rmj_determinize_order(uint64_t seed, uint64_t global_game, uint32_t seat, uint32_t m, uint32_t* perm /*[m]*/);
/* rmj_determinize_device / rmj_determinize with flags (RMJ_DETF_*): flags = 0 is the call above, byte for byte, and launches or allocates
 * nothing else.  RMJ_ERR_ARG for an unknown flag bit as well. */
int rmj_determinize_ex_device(rmj_handle h, const int32_t* d_index, uint32_t rows, const uint32_t* d_count, const RmjDeterminize* p, uint32_t flags);
int rmj_determinize_ex(rmj_handle h, const int32_t* index, uint32_t rows, const RmjDeterminize* p, uint32_t flags);
/* The key of the exchange (hand slot i < 16, partner j < 256) in step k < 16 of opponent r's (r < 3) walk for viewpoint seat < 4, from the
 * code the kernel runs; host only, needs no GPU.  RMJ_ERR_ARG outside these ranges or for a null key. */
int rmj_determinize_swap_key(uint64_t seed, uint64_t global_game, uint32_t seat, uint32_t r, uint32_t k, uint32_t i, uint32_t j, uint64_t* key);

/* shanten.rs:244-261 calculate_shanten / :470-484 calculate_shanten_3p over raw 34-histograms
 * (len_div3 = tile count / 3; -1 = complete hand).  Tables are generated at first use, on the host. */
int rmj_shanten(int device, const uint8_t* counts /*[n][34]*/, uint32_t n, int sanma, int8_t* out /*[n]*/);

/* shanten.rs:304-327 calculate_effective_tiles_with_discard / :525-548 _3p_with_discard: number of tile types whose
 * draw lowers the shanten (3n+1 hand), or the best such count over the discards that do not raise it (3n+2 hand).
 * The reference takes 136-ids and panics on a 3n hand; only types matter, a 3n hand yields 0xFFFFFFFF. */
int rmj_effective_tiles(int device, const uint8_t* counts /*[n][34]*/, uint32_t n, int sanma, uint32_t* out /*[n]*/);
/* shanten.rs:331-405 calculate_best_ukeire / :552-626 _3p: best, over the discards that do not raise the shanten, of the
 * number of live tiles (4 - visible - held, saturating) whose draw lowers it. */
int rmj_best_ukeire(int device, const uint8_t* counts /*[n][34]*/, const uint8_t* visible /*[n][34]*/, uint32_t n, int sanma,
                    uint32_t* out /*[n]*/);

/* ------------------------------------------------------------------ trainer-side device interface
 * Zero-copy views of the observation outputs for a policy that runs on the same GPU (riichienv-ml's PPO worker loop,
 * trainers/_ppo_worker.py:113-466, reads obs.mask() / obs.encode() per game on the host).  The pointers stay valid until
 * rmj_destroy; their contents are rewritten by every step / reset / apply call, in order, on `stream`. */
typedef struct RmjDeviceViews {
    uint32_t n_games, reserved;
    const uint32_t* status;   /* [n]        active_mask | phase << 8 | is_done << 16 */
    const uint8_t* nlegal;    /* [n][4]     */
    const uint64_t* legal;    /* [n][4][64] packed actions */
    const uint8_t* mask;      /* [n][4][82] action-id mask (first 60 ids in 3P) */
    const uint64_t* waits;    /* [n][4]     34-bit wait masks */
    void* stream;             /* hipStream_t of the handle */
} RmjDeviceViews;
int rmj_device_views(rmj_handle h, RmjDeviceViews* out);
/* step with the policy's action ids ([n][4] int32 on the device, -1 = no action): Observation.find_action
 * (observation/python.rs:119-122) + RiichiEnv.step; auto_reset != 0 restarts finished games like rmj_step_random */
int rmj_step_ids_device(rmj_handle h, const int32_t* d_action_ids, int auto_reset);
/* rmj_step_ids_device + rmj_encode_device(h, 2, d_out) as ONE launch: the step under the policy's ids, then Observation.encode() of
 * the seats that are to act next into the resident tensor d_out [n][4][74][34 | 27] (rows of the other seats untouched) - the
 * trainer loop's iteration (riichienv-ml trainers/_ppo_worker.py:151-239: step, then obs.encode() of the returned observations)
 * with one launch gap instead of two. */
int rmj_step_ids_encode_device(rmj_handle h, const int32_t* d_action_ids, int auto_reset, float* d_out);
/* rmj_sample_ids_device(h, d_logits, stride, seed, d_ids) + rmj_step_ids_encode_device(h, d_ids, auto_reset, d_out) as ONE launch (round 5):
 * every wave draws the ids of its own four games from the policy's logits (the same keyed draw: the ids are the ones the two calls
 * produce, and they are written to d_ids [n][4] for the caller's log-probabilities), steps under them and encodes the seats that act
 * next - the whole environment side of a trainer iteration (trainers/_ppo_worker.py:151-239) between two policy forward passes.
 * Non-finite logits are drawn as rmj_sample_ids_device describes. */
int rmj_step_sample_encode_device(rmj_handle h, const float* d_logits, uint32_t stride, uint64_t seed, int auto_reset, int32_t* d_ids, float* d_out);
/* Masked categorical sampling for a policy on the same GPU (what riichienv-ml's PPO worker does per game on the host with
 * obs.mask(), trainers/_ppo_worker.py:164-239): for every seat that is to act, one action id drawn from
 * softmax(logits) restricted to the seat's legal ids (Gumbel-max on the resident mask slab); d_logits [n][4][stride] f32 on
 * the device (stride >= 82 / 60; masked entries are never read as candidates), NULL = uniform over the legal ids.
 * d_ids [n][4] int32, -1 for seats that do not act: the input of rmj_step_ids_device.  Counter-based noise: the same
 * (seed, state) gives the same ids.  Asynchronous on the handle's stream.
 * Non-finite logits (here and in rmj_step_sample_encode_device): a -inf or NaN logit is never drawn while a finite one is legal;
 * if every legal id is -inf or NaN, the lowest legal id is drawn; among several +inf logits the lowest of them wins.  The noise
 * u of every id lies strictly inside (0, 1), so every finite logit gets a finite key. */
int rmj_sample_ids_device(rmj_handle h, const float* d_logits, uint32_t stride, uint64_t seed, int32_t* d_ids);
/* Action ids of one step when ONE seat per game learns (riichienv-ml trainers/_ppo_worker.py:164-239: the hero samples from the model,
 * the other seats take `opp_logits.masked_fill(~mask, -1e9).argmax`; :393-466 evaluate_episodes: every seat takes the arg-max).
 * As rmj_sample_ids_device plus d_hero [n] u8: seat d_hero[g] of game g gets the keyed Gumbel draw of rmj_sample_ids_device, unchanged
 * (the same (seed, state) gives the id that call gives that seat); every other seat that is to act gets the arg-max of its logits over
 * its legal ids - ties to the lowest id; a NaN or -inf logit is never chosen while a finite or +inf one is legal; if none is, the
 * lowest legal id (the sampler's rules above).  d_hero[g] = 255: every seat of that game takes the arg-max.  d_hero = NULL: every
 * seat samples (identical to rmj_sample_ids_device).  d_logits = NULL: all logits equal.  Cells the sampler never reads are not read.
 * Asynchronous on the handle's stream. */
int rmj_select_ids_device(rmj_handle h, const float* d_logits, uint32_t stride, uint64_t seed, const uint8_t* d_hero, int32_t* d_ids);

/* ------------------------------------------------------------------ PPO transition collector
 * What riichienv-ml's PPO worker returns (trainers/_ppo_worker.py:129-391 collect_episodes): the transitions of one hero seat per
 * game - features [N][C][W] f32, mask [N][A] u8, action [N] i64, log_prob, advantage, return [N] f32 - cut into one trajectory per
 * kyoku, with the generalised advantage estimate run backwards over each kyoku and the kyoku's reward paid on its last decision.
 * A collector is bound to a handle and owns a pool of `capacity` transitions (capacity x (C x W x 4 + A + 45) bytes of device memory:
 * the caller's decision; what does not fit is counted, never silently lost).  All calls are asynchronous on the handle's stream
 * and take device pointers; only rmj_ppo_counts waits.  One iteration of the worker's loop:
 *     obs batch -> policy -> rmj_select_ids_device -> rmj_ppo_record_device -> step (+ next obs batch) -> rmj_round_track_device
 *     -> the caller's reward -> rmj_ppo_close_device;   at the end rmj_ppo_emit_device. */
typedef struct RmjPpoConfig {
    int32_t features;     /* RMJ_FEATURES_*: the rows the pool stores (C x W of the handle's mode) */
    uint32_t capacity;    /* transitions */
    double gamma;         /* discount (_ppo_worker.py gamma) */
    double gae_lambda;
} RmjPpoConfig;
typedef struct rmj_ppo* rmj_ppo_handle;
/* RMJ_ERR_ARG for a feature set the handle cannot serve (DISCARD_SHANTEN in 3P), a zero capacity or a missing pointer.  The
 * collector lives until rmj_ppo_destroy or the handle's rmj_destroy, whichever comes first. */
int rmj_ppo_create(rmj_handle h, const RmjPpoConfig* cfg, rmj_ppo_handle* out);
int rmj_ppo_destroy(rmj_ppo_handle p);
/* Between the policy's forward pass and the step (_ppo_worker.py:164-199): for every game whose hero is to act
 * (d_ids[g][d_hero[g]] >= 0; a hero of 255 never records) one transition is appended - the feature row of (game, hero) from the
 * observation batch `b` the policy just read (either layout of RmjObsBatch, the collector's feature set), the seat's mask bytes, the
 * action id, the policy's value, and log_prob = log_softmax(masked_fill(logits, ~mask, -1e9))[action] (:175-182) computed in f32 from
 * the row's logits.  d_logits / d_values are laid out like the observation rows: dense [n][4][logits_stride] / [n][4], compact
 * [rows][logits_stride] / [rows] by compact slot.  Slots are handed out in (call, game) order.  When the pool is full nothing is
 * written: the transition is counted as overflowed and the game's open trajectory is marked broken, so that a trajectory with a hole
 * is never emitted.  The same holds for a hero whose row is missing from a compact batch that was too small. */
int rmj_ppo_record_device(rmj_ppo_handle p, const RmjObsBatch* b, const uint8_t* d_hero, const int32_t* d_ids, const float* d_logits,
                          uint32_t logits_stride, const float* d_values);
/* After the step and the caller's reward computation (_ppo_worker.py:240-281): d_ended [n] u8, non-zero = the hero's open trajectory
 * of this game ends here (rmj_round_track_device's `ended`: a renchan is a boundary; or a change of kyoku_idx / the game's end, the
 * worker's own rule), d_reward [n] f32 = the hero's reward for that kyoku.  The trajectory's advantages and returns are computed as
 * :314-326 does - float64 over the f32 values and reward, the worker's order of operations, no fused multiply-add, rounded to f32
 * once (:350-351): the worker's bits - and its transitions become valid.  Empty trajectories are skipped (:307-308), broken ones
 * dropped. */
int rmj_ppo_close_device(rmj_ppo_handle p, const uint8_t* d_ended, const float* d_reward);
/* The worker's flattening (:328-353): the valid transitions, in pool order, into the caller's arrays (`rows` rows each; action as
 * int64 like the worker's).  d_count [2] u32: [0] the number of valid transitions (when it exceeds `rows` only the first `rows` were
 * written), [1] the slots left out because their trajectory was still open or broken. */
typedef struct RmjPpoBatch {
    float* d_features;    /* [rows][C][W] */
    uint8_t* d_mask;      /* [rows][A], A = 82 (60 in 3P) */
    int64_t* d_action;
    float* d_log_prob;
    float* d_advantage;
    float* d_return;
    uint32_t* d_count;    /* [2] */
    uint32_t rows, reserved;
} RmjPpoBatch;
int rmj_ppo_emit_device(rmj_ppo_handle p, const RmjPpoBatch* out);
/* The pool itself, without a copy: slot s < fill is a transition, `valid[s]` says whether its trajectory was closed complete.
 * row_stride: floats from one feature row to the next (C x W rounded up to 4).  game / serial / t / prev: the slot's game, the
 * game's trajectory serial, the position in the trajectory, the slot of the trajectory's previous transition (-1: first).  seg_len /
 * seg_reward: at the LAST slot of a closed trajectory its length and reward, 0 elsewhere (the worker's kyoku statistics).  counters:
 * device u32 [5] = the fields of RmjPpoCounts except `open`.  Valid until the collector is destroyed. */
typedef struct RmjPpoViews {
    uint32_t capacity, row_stride, action_space, reserved;
    const float* features;
    const uint8_t* mask;
    const int32_t* action;
    const float *value, *log_prob, *advantage, *ret;
    const uint8_t* valid;
    const int32_t *game, *t, *prev, *seg_len;
    const uint32_t* serial;
    const float* seg_reward;
    const uint32_t* counters;
    const uint32_t* open_len;   /* [n_games] transitions of every game's open trajectory */
} RmjPpoViews;
int rmj_ppo_views(rmj_ppo_handle p, RmjPpoViews* out);
/* Waits for the handle's stream.  fill = valid + open + dropped. */
typedef struct RmjPpoCounts {
    uint32_t fill;        /* slots in use */
    uint32_t valid;       /* transitions of trajectories closed complete */
    uint32_t dropped;     /* transitions of broken trajectories that were closed: never emitted */
    uint32_t overflowed;  /* transitions that found no slot (or no observation row) */
    uint32_t segments;    /* trajectories closed complete */
    uint32_t open;        /* transitions of trajectories still open */
} RmjPpoCounts;
int rmj_ppo_counts(rmj_ppo_handle p, RmjPpoCounts* out);
/* Empties the pool and forgets the open trajectories (a new collect_episodes call). */
int rmj_ppo_clear(rmj_ppo_handle p);

/* ------------------------------------------------------------------ log sample builder
 * What riichienv-ml's MCDataset yields from MJAI logs (datasets/mjai_logs.py:62-129) - per decision of every seat the feature row, the
 * action id, the decayed return G_t = reward x gamma ** (T - t - 1), the action mask and the seat's rank in the kyoku's end scores -
 * built on the device: M logs are replayed in lock-step in the n <= M games of a handle, with no host work per event and no host
 * synchronisation inside the replay.
 *
 * A log set is the logs' events as ONE resident array of records, events[total][3] as rmj_apply_events takes them (the host packs
 * every MJAI event once; riichienv_amd/abi.py event_records_from_mjai), with offsets[n_logs + 1] = the first event of every log.  A
 * kyoku of a log is numbered by the start_kyoku events of the log so far (the first kyoku is 1); its row in the per-kyoku tables
 * (reward, end scores) is kyoku_offsets[log] + kyoku - 1, kyoku_offsets [n_logs + 1] from the info call (NULL: not wanted). */
typedef struct rmj_logset* rmj_logset_handle;
typedef struct RmjLogsetInfo {
    uint32_t n_logs, n_events, n_kyokus, longest_log;
} RmjLogsetInfo;
int rmj_logset_create(int device, const RmjEvent* events /*[total][3]*/, const uint32_t* offsets /*[n_logs + 1]*/, uint32_t n_logs, rmj_logset_handle* out);
int rmj_logset_destroy(rmj_logset_handle s);
int rmj_logset_info(rmj_logset_handle s, RmjLogsetInfo* out, uint32_t* kyoku_offsets /*[n_logs + 1]*/);
/* A log set straight from MJAI JSONL text, parsed on the device (csrc/rmj_evparse.h, csrc/rmj_logtext.hip.h): log i is the bytes
 * text[ranges[i][0] .. ranges[i][1]), one JSON object per line ('\n'; the last line may lack it; lines that are empty after trimming
 * spaces, tabs and a trailing '\r' are not events).  The ranges need not be contiguous or ordered (leaving a range out drops a log); a
 * log is at most 4 GiB - 1 of text.  Every line becomes the three records abi.event_records_from_mjai gives for it (num_players: 3 or 4,
 * the seats whose tehais are read; RMJ_LOGTEXT_MASKED_OK: unmappable tile names read as tile 0), and the set also holds, resident, the
 * per-kyoku score tables of datasets.kyoku_tables (start / end scores [n_kyokus][4] int32), every log's decision-event count and its
 * status: RMJ_LOGTEXT_OK, or the status of its first line that did not parse (error_line: that line, numbered from 1, blank lines
 * included; 0 when the log is fine or failed in the kyoku walk).  A line that fails gives three NONE records; a set with failed logs is
 * still returned.  Statuses (never silently different from the host packer: csrc/rmj_evparse.h lists what is declined):
 * ERR_* where json.loads or the packer raises, UNSUPPORTED for valid input the parser declines to interpret.
 * Without RMJ_LOGTEXT_ON_DEVICE text and ranges are host memory (the bytes between the lowest begin and the highest end are uploaded in
 * one copy); with it both are device pointers.  Synchronous like rmj_logset_create: the set is complete on return, the temporaries are
 * freed, and rmj_logset_info / rmj_logreplay_create / rmj_logreplay_assign work on it unchanged.  RMJ_ERR_RANGE when the logs hold more
 * than UINT32_MAX events or a log is 4 GiB or longer; RMJ_ERR_ARG for a range with end < begin, num_players not 3 or 4, an unknown flag. */
#define RMJ_LOGTEXT_OK 0
#define RMJ_LOGTEXT_UNSUPPORTED 1  /* valid JSON the device parser declines to interpret (escaped key, 1.5 as actor, duplicate key, ...) */
#define RMJ_LOGTEXT_ERR_JSON 2     /* not a JSON object (json.loads raises) */
#define RMJ_LOGTEXT_ERR_KEY 3      /* a key the event's type requires is missing */
#define RMJ_LOGTEXT_ERR_TEHAI 4    /* start_kyoku: a tehai that does not hold 13 tiles */
#define RMJ_LOGTEXT_ERR_TILE 5     /* a tile name that maps to nothing (without RMJ_LOGTEXT_MASKED_OK) */
#define RMJ_LOGTEXT_ERR_VALUE 6    /* null where the event's type requires a value */
#define RMJ_LOGTEXT_ERR_REPLAY 7   /* the kyoku walk (MjaiReplay.from_events) raises: an actor that is no seat of the kyoku, a call without target */
#define RMJ_LOGTEXT_ON_DEVICE 1u
#define RMJ_LOGTEXT_MASKED_OK 2u
int rmj_logset_create_from_text(int device, const uint8_t* text, const uint64_t* ranges /*[n_logs][2] begin, end*/, uint32_t n_logs, uint32_t num_players,
                                uint32_t flags, rmj_logset_handle* out);
/* Device pointers into a set.  The score tables, status, error_line and decisions are NULL for a set made by rmj_logset_create. */
typedef struct RmjLogsetViews {
    const RmjEvent* events;          /* [n_events][3] */
    const uint32_t* offsets;         /* [n_logs + 1] */
    const uint32_t* kyoku_offsets;   /* [n_logs + 1] */
    const int32_t* start_scores;     /* [n_kyokus][4] */
    const int32_t* end_scores;       /* [n_kyokus][4] */
    const uint8_t* status;           /* [n_logs] RMJ_LOGTEXT_* */
    const uint32_t* error_line;      /* [n_logs] */
    const uint32_t* decisions;       /* [n_logs] events of a decision type (dahai chi pon daiminkan kan ankan kakan reach hora kita ryukyoku) */
} RmjLogsetViews;
int rmj_logset_views(rmj_logset_handle s, RmjLogsetViews* out);
/* Host copies of a text set's per-log results (any may be NULL); RMJ_ERR_ARG for status / error_line / decisions of a set made by
 * rmj_logset_create. */
int rmj_logset_status(rmj_logset_handle s, uint8_t* status /*[n_logs]*/, uint32_t* error_line /*[n_logs]*/, uint32_t* decisions /*[n_logs]*/,
                      uint32_t* offsets /*[n_logs + 1]*/);
/* GRP rank-model rows: the input of riichienv-ml's rank model (datasets/grp_dataset.py GrpReplayDataset._encode_features, the same
 * layout as RewardPredictor.calc_all_player_rewards) for every seat of a round.  The row of seat p, n = num_players (3 or 4), is
 * 4n + 4 float32:
 *     init[0..n) / S, end[0..n) / S, delta[0..n) / 12000, chang / 3, ju / 3, ben / 4, liqibang / 4, onehot(p)[0..n)
 * S = 25000 (4P) or 35000 (3P), delta = end - init.  Every quotient is the float64 division of the integer by the constant rounded
 * once to float32 (Python's int / float, then np.float32): bit-equal to the reference's rows.
 * Both calls are asynchronous on `hip_stream` (a hipStream_t, as rmj_set_stream takes it; NULL = the null stream), allocate nothing and
 * wait for nothing.  Every table pointer is a device pointer, 16-byte aligned.
 *
 * rmj_grp_rows_device: the pure form - init, delta, meta int32 [rows][4] -> x [rows][n][4n + 4]; meta = (chang, ju, ben, liqibang),
 * what rmj_round_track_device writes (the live / PPO path: init = the scores when the round was dealt, end = init + delta). */
int rmj_grp_rows_device(int device, const int32_t* d_init, const int32_t* d_delta, const int32_t* d_meta, uint32_t rows, uint32_t num_players, float* d_x,
                        void* hip_stream);
/* rmj_logset_grp_device: one row block per kyoku of a log set, in table order kyoku_offsets[log] + kyoku - 1.  meta is read from the
 * kyoku's START_KYOKU record: chang = the bakaze index, ju = kyoku - 1 (-1 for "kyoku": 0, like the host), ben = honba, liqibang = both
 * kyotaku bytes.  rank = the seat's place (0 = first) in the end scores of its LOG'S LAST kyoku - GrpReplayDataset's label: a stable
 * descending sort, ties to the lower seat - or 255 for every kyoku of a log whose status is not RMJ_LOGTEXT_OK (x is still written, from
 * whatever the tables hold).  log_of = the kyoku's log.  A log without a kyoku contributes nothing.  start_scores / end_scores
 * [n_kyokus][4]: NULL = the set's own tables (a set parsed from text); a set made by rmj_logset_create has none and RMJ_ERR_ARG is
 * returned when they are NULL.  Any output may be NULL, except that x needs meta. */
typedef struct RmjGrpOut {
    int32_t* meta;      /* [n_kyokus][4] chang, ju, ben, liqibang */
    float* x;           /* [n_kyokus][n][4n + 4] */
    uint8_t* rank;      /* [n_kyokus][n] */
    uint32_t* log_of;   /* [n_kyokus] */
} RmjGrpOut;
int rmj_logset_grp_device(rmj_logset_handle s, uint32_t num_players, const int32_t* d_start_scores, const int32_t* d_end_scores, const RmjGrpOut* out,
                          void* hip_stream);
/* Play statistics: how every seat played every kyoku of a log set - int32 rows[n_kyokus][4][RMJ_PLAYSTAT_COLUMNS], one row block per
 * kyoku in table order kyoku_offsets[log] + kyoku - 1.  A kyoku runs from its START_KYOKU record up to the next START_KYOKU of the same
 * log, or to the log's end; events before a log's first START_KYOKU belong to no row.  Only type, actor and flags of an event's first
 * record are read (and the oya of a START_KYOKU); an event whose actor >= num_players is skipped as if its type were NONE.
 * Hora records carry no target, so who dealt in is derived from the stream.  A tile event is a TSUMO, DAHAI, KAKAN, ANKAN or KITA; for a
 * HORA of seat a, with L the last tile event before it in the same kyoku: L a TSUMO by a - a tsumo win; else L by a seat x != a - x dealt
 * in (ron, chankan, kokushi on an ankan); else (no L, or another tile event of a's own) - a win only.
 * Columns of seat p: */
#define RMJ_PLAYSTAT_COLUMNS 16
#define RMJ_PLAYSTAT_WIN 0              /* HORA events of p */
#define RMJ_PLAYSTAT_WIN_TSUMO 1        /* those that are tsumo wins */
#define RMJ_PLAYSTAT_DEAL_IN 2          /* HORA events of other seats into which p dealt (a double ron counts 2) */
#define RMJ_PLAYSTAT_RIICHI 3           /* REACH events of p */
#define RMJ_PLAYSTAT_RIICHI_ACCEPTED 4  /* REACH_ACCEPTED events of p */
#define RMJ_PLAYSTAT_RIICHI_TURN 5      /* 1 + the DAHAI events of p before its first REACH of the kyoku; 0 without one */
#define RMJ_PLAYSTAT_CALLS 6            /* CHI + PON + DAIMINKAN of p */
#define RMJ_PLAYSTAT_CHI 7
#define RMJ_PLAYSTAT_PON 8
#define RMJ_PLAYSTAT_KANS 9             /* DAIMINKAN + ANKAN + KAKAN of p */
#define RMJ_PLAYSTAT_KITA 10
#define RMJ_PLAYSTAT_DISCARDS 11        /* DAHAI events of p */
#define RMJ_PLAYSTAT_TSUMOGIRI 12       /* of those, the ones with flags bit 0 */
#define RMJ_PLAYSTAT_WIN_TURN 13        /* the DAHAI events of p before its first HORA of the kyoku; 0 without one */
#define RMJ_PLAYSTAT_DEALER 14          /* 1 if the kyoku's oya is p */
#define RMJ_PLAYSTAT_END 15             /* the same in every seat < num_players: bit 0 a HORA occurred, bit 1 a RYUKYOKU occurred */
/* Seats >= num_players are all zero (END included).  Every kyoku row of a log whose status is not RMJ_LOGTEXT_OK holds -1 in all 64
 * words, so a sum that forgot to mask those rows is visibly wrong.  Every word of the table is written exactly once per call: the
 * caller does not clear it.  Asynchronous on `hip_stream` (NULL = the null stream), allocates nothing, waits for nothing; works on both
 * kinds of set and needs no score tables.  RMJ_ERR_ARG for a null set and for num_players other than 3 or 4.  A set without kyokus then
 * returns RMJ_OK without a launch and without looking at d_rows (an empty table may have a null pointer).  Otherwise RMJ_ERR_ARG for
 * null rows and for rows that are not 16-byte aligned. */
int rmj_logset_playstats_device(rmj_logset_handle s, uint32_t num_players, int32_t* d_rows /*[n_kyokus][4][16]*/, void* hip_stream);
/* Which slot replays which logs (host only, no device needed): the logs are handed out in log order, each to the slot that is free
 * first when every event takes one step, ties to the lowest slot - a pure function of (n_logs, n_slots, the logs' lengths), so the
 * order of the samples is the same run after run.  slot_of_log [n_logs]; slot s replays slot_logs[slot_first[s] .. slot_first[s + 1])
 * in that order (slot_logs [n_logs], slot_first [n_slots + 1]); *steps = the events of the busiest slot = the steps of a whole replay.
 * Any output may be NULL.  RMJ_ERR_ARG unless 1 <= n_slots <= n_logs (or both are 0). */
int rmj_logreplay_assign(const uint32_t* offsets, uint32_t n_logs, uint32_t n_slots, uint32_t* slot_of_log, uint32_t* slot_logs, uint32_t* slot_first,
                         uint32_t* steps);
#define RMJ_LOGREPLAY_INCLUDE_PASS 1u        /* the Pass of every seat that was offered a claim and let it go is a sample */
#define RMJ_LOGREPLAY_SKIP_SINGLE_ACTION 2u  /* a decision over a list of at most one action is no sample (LogKyoku.steps' default) */
#define RMJ_LOGREPLAY_HIDDEN 4u              /* every pool slot also keeps its hidden-hand record and event index: rmj_logreplay_emit_hidden_device */
#define RMJ_LOGREPLAY_DANGER 8u              /* every pool slot also keeps its deal-in danger record: rmj_logreplay_emit_danger_device */
#define RMJ_LOGREPLAY_DTABLE 16u             /* every pool slot also keeps its discard efficiency record: rmj_logreplay_emit_dtable_device */
typedef struct RmjLogReplayConfig {
    int32_t features;           /* RMJ_FEATURES_*: the rows the pool stores */
    uint32_t capacity;          /* samples: capacity x (C x W x 4 + A + 52) bytes of device memory, + 152 with RMJ_LOGREPLAY_HIDDEN, + 224 with RMJ_LOGREPLAY_DANGER, + 112 with RMJ_LOGREPLAY_DTABLE */
    uint32_t flags;             /* RMJ_LOGREPLAY_* */
    uint32_t n_powers;
    double gamma;
    const double* gamma_powers; /* host array [n_powers], P[k] = gamma ** k as the trainer's own arithmetic gives it (Python: gamma ** k), at
                                   least longest_log + 1 entries: a return is ONE float64 product reward x P[T - t - 1], so it has the
                                   dataset's bits without a device pow.  NULL: the library fills the table with pow(gamma, k). */
} RmjLogReplayConfig;
typedef struct rmj_logreplay* rmj_logreplay_handle;
/* The handle's games are the slots (n_slots = n_games <= n_logs, else RMJ_ERR_ARG; so are a zero capacity, an unknown feature set or
 * flag, DISCARD_SHANTEN in 3P).  The handle should be used for nothing else while a replay is under way: start_kyoku events rewrite
 * its games.  The builder lives until its destroy call or the handle's rmj_destroy; the log set must outlive it. */
int rmj_logreplay_create(rmj_handle h, rmj_logset_handle set, const RmjLogReplayConfig* cfg, rmj_logreplay_handle* out);
int rmj_logreplay_destroy(rmj_logreplay_handle r);
/* n_steps steps of the replay (0 = to the end), asynchronous on the handle's stream; *steps_left (may be NULL) = what remains.  A step
 * takes the next event of every slot's log: the decisions it stands for are matched on the device against the published legal lists
 * (Observation.select_action_from_mjai, observation/mjai_select.rs:88-194: the first match in list order; the tsumogiri / drawn-tile
 * rule of a dahai; consumed tiles compared as a multiset of MJAI names, so red fives are distinct; hora = Tsumo or Ron; ryukyoku =
 * KyushuKyuhai), together with what the reference's log walker yields without a direct match - the Pass decisions (flag), the Ron on
 * a robbed kakan / ankan, which the published lists do not hold (replay/mod.rs:483-527) - and every sample is written to the pool:
 * feature row, mask, action id, packed action, (log, kyoku, seat, t) with t the position in the seat's trajectory of that kyoku.
 * Then the event is applied with RMJ_EVF_REPLAY_PASS.  Pool slots are handed out in (step, slot, decision) order, passes first, highest
 * seat first (LogKyoku.steps' order).  When the pool is full nothing is written: the sample is counted as overflowed and its
 * trajectory marked broken.  A log in which a decision event finds no match in the list its actor is offered is marked failed (a
 * status word, no trap) and left at once; its slot goes on with its next log (mjai_logs.py:119-122 drops such a file whole).
 * NOT detected: an event that does not fit the state in any other way (a decision event by a seat that is not to act, a tsumo out of
 * turn, a meld from tiles the hand does not hold when no list is offered).  The event handler reports no error, like the reference's
 * apply_mjai_event; such an event is applied as rmj_apply_events applies it and the log counts as complete.
 * The records carry less than the MJAI text, and matching follows the records: a dahai without a tsumogiri field reads as
 * tsumogiri = false (select_action_from_mjai skips the drawn-tile rule when the field is absent: on such third-party logs the twin
 * of the same name may be picked), a kakan is matched by its tile name without its consumed tiles, and the seat a robbed kan is
 * taken from is the log's previous actor, not the hora's target field.  On logs that a game produced these agree. */
int rmj_logreplay_run_device(rmj_logreplay_handle r, uint32_t n_steps, uint32_t* steps_left);
/* Returns and ranks of the samples in the pool: d_reward [n_kyokus][4] f64 = the reward of (kyoku row, seat) - where
 * RewardPredictor.calc_all_player_rewards plugs in - and d_end_scores [n_kyokus][4] i32 = the kyoku's end scores; return64 = reward x
 * P[T - t - 1] (T = the samples of the trajectory), `ret` = that rounded to f32, rank = the seat's place in a stable descending sort
 * of the end scores (mjai_logs.py:14-17: ties to the lower seat). */
int rmj_logreplay_finalize_device(rmj_logreplay_handle r, const double* d_reward, const int32_t* d_end_scores);
/* The samples of the logs that were replayed to their end, minus the trajectories that lost a sample to a full pool, in pool order,
 * into the caller's device arrays of `rows` rows.  d_count [2] u32: [0] the samples that qualify (when above `rows` only the first
 * `rows` were written), [1] the pool slots left out (failed or unfinished logs, broken trajectories). */
typedef struct RmjLogBatch {
    float* d_features;    /* [rows][C][W] */
    uint8_t* d_mask;      /* [rows][A] */
    int64_t* d_action;    /* action id */
    uint64_t* d_packed;   /* packed action */
    float* d_return;
    double* d_return64;
    int64_t* d_rank;
    int32_t *d_log, *d_kyoku, *d_seat, *d_t;
    uint32_t* d_count;    /* [2] */
    uint32_t rows, reserved;
} RmjLogBatch;
int rmj_logreplay_emit_device(rmj_logreplay_handle r, const RmjLogBatch* out);
/* The pool itself, without a copy (slot s < fill).  row_stride: floats from one feature row to the next; steps: the steps of a whole
 * replay.  log_status [n_logs] u8: 0 not finished, 1 replayed to its end, 2 failed; traj_len / traj_broken [n_kyokus][4]; counters:
 * device u32 [6] = fill, overflowed, failed logs, (internal), decisions, events applied. */
typedef struct RmjLogReplayViews {
    uint32_t capacity, row_stride, action_space, steps;
    const float* features;
    const uint8_t* mask;
    const int32_t* action;
    const uint64_t* packed;
    const float* ret;
    const double* ret64;
    const int32_t *rank, *log, *kyoku, *seat, *t;
    const uint8_t* log_status;
    const uint32_t* traj_len;
    const uint8_t* traj_broken;
    const uint32_t* counters;
} RmjLogReplayViews;
int rmj_logreplay_views(rmj_logreplay_handle r, RmjLogReplayViews* out);
/* Waits for the handle's stream. */
typedef struct RmjLogReplayCounts {
    uint32_t fill;           /* pool slots in use */
    uint32_t overflowed;     /* samples that found no slot */
    uint32_t failed_logs;
    uint32_t complete_logs;
    uint32_t decisions;      /* samples matched (fill + overflowed) */
    uint32_t events;         /* events taken from the stream */
    uint32_t steps_done, steps_left;
} RmjLogReplayCounts;
int rmj_logreplay_counts(rmj_logreplay_handle r, RmjLogReplayCounts* out);
/* Empties the pool and rewinds every slot to its first log (the handle's games are rewritten by the logs' own start events). */
int rmj_logreplay_clear(rmj_logreplay_handle r);
/* RMJ_LOGREPLAY_HIDDEN: every sample also gets the hidden-hand row of (its slot's game, the deciding seat) - the fields of
 * rmj_hidden_targets_device - and `event`, the index in its log of the event the decision precedes.  Both are taken at the moment
 * the feature row is: from the state before the step's event is applied, by a kernel of their own between the step's record and apply
 * launches (without the flag the replay launches what it always did and allocates nothing more).  A sample that found no pool slot
 * has no record either.  The records lie in a second allocation of capacity x 152 bytes: per slot three opponents of 48 bytes (waits
 * u64 at 0, hand [34] u8 at 8, shanten i8 at 42, flags u8 at 43), then the event i32 at 144.  Meaningless on logs with masked ("?")
 * tiles: the caller keeps such sets away (the records do not say how a set was made).
 * The emit call writes the records of the samples rmj_logreplay_emit_device emits, to the same rows in the same order: d_opp_* as
 * in RmjHiddenOut, d_event [rows] i32; rows beyond `rows` are dropped like there.  Call it while the pool is as the other emit call
 * saw it.  RMJ_ERR_ARG for a builder made without the flag. */
typedef struct RmjLogHiddenBatch {
    uint8_t* d_opp_hand;     /* [rows][3][34] */
    int8_t* d_opp_shanten;   /* [rows][3] */
    uint64_t* d_opp_waits;   /* [rows][3] */
    uint8_t* d_opp_flags;    /* [rows][3] */
    int32_t* d_event;        /* [rows] */
    uint32_t rows, reserved;
} RmjLogHiddenBatch;
int rmj_logreplay_emit_hidden_device(rmj_logreplay_handle r, const RmjLogHiddenBatch* out);
/* The records themselves, without a copy (slot s < fill at records + s x record_bytes); records = NULL for a builder made without
 * the flag. */
typedef struct RmjLogHiddenViews {
    uint32_t capacity, record_bytes;
    const uint8_t* records;
} RmjLogHiddenViews;
int rmj_logreplay_hidden_views(rmj_logreplay_handle r, RmjLogHiddenViews* out);
/* RMJ_LOGREPLAY_DANGER: every sample also gets the deal-in danger row of (its slot's game, the deciding seat) - d_danger of
 * rmj_danger_targets_device without RMJ_DANGER_URA (logs carry no wall) - taken where the hidden record is: from the state before the
 * step's event is applied, by a kernel of its own right behind the hidden one (without the flag the replay launches what it always did
 * and allocates nothing more).  Independent of RMJ_LOGREPLAY_HIDDEN.  The records lie in an allocation of their own of capacity x 224
 * bytes: per slot [3][37] u16 in hundreds of points (every ron value is a multiple of 100).  Meaningless on logs with masked tiles.
 * The emit call widens the records of the samples rmj_logreplay_emit_device emits to i32 points, in the same rows in the same order;
 * rows beyond `rows` are dropped like there.  RMJ_ERR_ARG for a builder made without the flag. */
typedef struct RmjLogDangerBatch {
    int32_t* d_danger;       /* [rows][3][37] */
    uint32_t rows, reserved;
} RmjLogDangerBatch;
int rmj_logreplay_emit_danger_device(rmj_logreplay_handle r, const RmjLogDangerBatch* out);
/* RMJ_LOGREPLAY_DTABLE: every sample also gets the discard efficiency row of (its slot's game, the deciding seat) - d_shanten, d_accept
 * and d_ukeire of rmj_discard_table_device - taken where the hidden record is: from the state before the step's event is applied, by a
 * kernel of its own behind the hidden and danger ones (without the flag the replay launches what it always did and allocates nothing
 * more).  Independent of the other record flags.  The records lie in an allocation of their own of capacity x 112 bytes: per slot three
 * byte arrays of 35 (shanten i8, accept u8, ukeire u8) and 7 spare bytes.  The masks are left out of the pool: 280 more bytes per slot
 * buy nothing a trainer needs (accept counts them; rmj_discard_table_device has them for a live row).  Meaningful only where the deciding
 * seat's own hand is known.  The emit call copies the records of the samples rmj_logreplay_emit_device emits to the same rows in the
 * same order; rows beyond `rows` are dropped like there.  RMJ_ERR_ARG for a builder made without the flag. */
typedef struct RmjLogDtableBatch {
    int8_t* d_shanten;       /* [rows][35] */
    uint8_t* d_accept;       /* [rows][35] */
    uint8_t* d_ukeire;       /* [rows][35] */
    uint32_t rows, reserved;
} RmjLogDtableBatch;
int rmj_logreplay_emit_dtable_device(rmj_logreplay_handle r, const RmjLogDtableBatch* out);

/* ------------------------------------------------------------------ log validation
 * A verdict for every log of a log set before samples are built from it (riichienv-ml validates a corpus one log at a time through
 * Python, scripts/validate_logs.py): a checking replay on the device, in the slots of a handle like the sample builder's, that records
 * no sample and allocates no pool.  Every log gets its FIRST finding - the one at the lowest event index, and at one event the lowest
 * code: code, event (the index of the offending MJAI event in the log, from 0), kyoku (the start_kyoku events of the log up to there),
 * seat (255: the event names none) and a detail word.  n = the number of players.
 *   OK
 *   PARSE               the set keeps the log with a text status other than RMJ_LOGTEXT_OK: it is not replayed; event = the set's
 *                       error line, detail = the status
 *   NO_START_KYOKU      an event other than start_game, start_kyoku, end_kyoku, end_game or NONE before the log's first start_kyoku
 *   AFTER_END           the open kyoku is over (a hora, ryukyoku or end_kyoku was applied) and the event is not hora, end_kyoku,
 *                       end_game, start_kyoku, start_game or NONE
 *   UNFINISHED          a start_kyoku, start_game or end_game arrives, or the log ends (event = the log's length), while a kyoku is
 *                       started and not over - how a log drained from a game in progress ends: the caller may accept the code
 *   ACTOR               tsumo dahai reach reach_accepted chi pon daiminkan ankan kakan hora (3P: kita) with actor >= n; chi pon
 *                       daiminkan with target >= n or target == actor; a start_kyoku with oya >= n (kyoku counts it, seat = 255).
 *                       Such an event is never applied: no game indexes a seat it does not have
 *   DRAW_OUT_OF_TURN    a tsumo by a seat other than the one due to draw: the oya after start_kyoku, (actor + 1) % n after a dahai,
 *                       the actor after daiminkan ankan kakan (3P: kita), nobody after tsumo chi pon
 *   NOT_OFFERED         the kyoku is open and the actor of a decision event (dahai chi pon daiminkan ankan kakan reach hora kita) is
 *                       offered no list: not among the active seats, or its published list is empty.  The Ron on a robbed kan, as
 *                       the sample builder recognises it, is exempt
 *   TILE_NOT_HELD       the actor's concealed hand does not hold the event's tile ids as a multiset: the tile of a dahai or kakan,
 *                       the first 2 consumed tiles of a chi or pon, 3 of a daiminkan, 4 of an ankan; detail = the tile id
 *   TILE_COUNT          at start_kyoku, tsumo or dora: among the dealt tiles, the dora markers and the draws of the kyoku so far a
 *                       tile type occurs more than 4 times (a red five counts to its type) or a red five more than once; detail = a
 *                       tile id of that name (the event's tile at tsumo / dora).  Masked logs ("?" read as tile 0) trip this
 *   NO_LEGAL_MATCH      the actor is offered a list and the event matches none of its entries (what fails a log in the sample builder)
 *   SCORE_CONTINUITY    the end scores of kyoku k - its start scores and what its hora / ryukyoku events move, computed as the kyoku
 *                       tables compute them for a log's last kyoku - differ from the start scores of kyoku k + 1: reported at the
 *                       start_kyoku of kyoku k + 1 with kyoku = k + 1, seat = the first seat that differs.  A ryukyoku's deltas are read
 *                       both ways, without the riichi deposits (converted Tenhou logs: the tables' reading) and with them (logs this
 *                       engine writes): a kyoku that fits either reading in every seat passes.  (The tables' own end column cannot
 *                       tell: for every kyoku but the last it IS the next start_kyoku's scores; a set parsed from text keeps these.)
 *   SCORE_CONSERVATION  sum(end - start) of kyoku k - end as the tables hold it, the start scores of kyoku k + 1 - is not
 *                       -1000 x (kyotaku[k + 1] - kyotaku[k]), kyotaku from the start_kyoku records; reported like SCORE_CONTINUITY;
 *                       detail = the sum
 * Not checked: a second or third hora of a multiple ron against an offer (the kyoku is over when it arrives), settlement amounts (the
 * records carry no ura markers), feature encodings. */
#define RMJ_LOGCHECK_OK 0
#define RMJ_LOGCHECK_PARSE 1
#define RMJ_LOGCHECK_NO_START_KYOKU 2
#define RMJ_LOGCHECK_AFTER_END 3
#define RMJ_LOGCHECK_UNFINISHED 4
#define RMJ_LOGCHECK_ACTOR 5
#define RMJ_LOGCHECK_DRAW_OUT_OF_TURN 6
#define RMJ_LOGCHECK_NOT_OFFERED 7
#define RMJ_LOGCHECK_TILE_NOT_HELD 8
#define RMJ_LOGCHECK_TILE_COUNT 9
#define RMJ_LOGCHECK_NO_LEGAL_MATCH 10
#define RMJ_LOGCHECK_SCORE_CONTINUITY 11
#define RMJ_LOGCHECK_SCORE_CONSERVATION 12
#define RMJ_LOGCHECK_CODES 13
#define RMJ_LOGCHECK_COUNTERS 16          /* words of the per-code counters */
#define RMJ_LOGCHECK_GUARDS 1u            /* create flag: RMJ_LOGCHECK_GUARD_WORDS words of RMJ_LOGCHECK_GUARD_WORD either side of every verdict array */
#define RMJ_LOGCHECK_GUARD_WORDS 64
#define RMJ_LOGCHECK_GUARD_WORD 0xA5C3F00Du
struct rmj_logcheck;
/* The name of a code ("TILE_NOT_HELD"), NULL for a number that is none. */
const char* rmj_logcheck_name(uint32_t code);
/* The first n_slots games of the handle are the slots (0 = all of them; else 1 <= n_slots <= the handle's games), at most one per log.
 * The handle should be used for nothing else while the validation is under way, and its game mode decides the number of players and
 * the rules the offers follow.  flags: RMJ_LOGCHECK_GUARDS or 0.  The checker lives until its destroy call (before the handle's
 * rmj_destroy); the log set must outlive it.  RMJ_ERR_ARG for a set on another device, an unknown flag, more slots than logs or games,
 * a set without logs. */
int rmj_logcheck_create(rmj_handle h, rmj_logset_handle set, uint32_t n_slots, uint32_t flags, struct rmj_logcheck** out);
int rmj_logcheck_destroy(struct rmj_logcheck* c);
/* The score tables (device pointers, i32) the two score checks read instead of the set's own - the start scores [n_kyokus][4], and
 * [n_kyokus][8] the end scores every kyoku's own events give in both readings (NOT the tables' end column, see SCORE_CONTINUITY): a
 * set made by rmj_logset_create holds none, and without this call those two checks are left out for it.  Read during
 * rmj_logcheck_run_device. */
int rmj_logcheck_set_scores(struct rmj_logcheck* c, const int32_t* d_start_scores /*[n_kyokus][4]*/, const int32_t* d_own_end_scores /*[n_kyokus][8]*/);
/* n_steps event indices of the validation (0 = to the end), asynchronous on the handle's stream: no host synchronisation, two launches
 * per event index (the checking pass, the event).  *steps_left (may be NULL) = what remains; the verdicts are complete at 0. */
int rmj_logcheck_run_device(struct rmj_logcheck* c, uint32_t n_steps, uint32_t* steps_left);
/* Device pointers to the verdicts: per log code, seat (u8), kyoku, event, detail (u32); counts [RMJ_LOGCHECK_COUNTERS] u32 = logs per code. */
typedef struct RmjLogCheckViews {
    uint32_t n_logs, steps;
    const uint8_t *code, *seat;
    const uint32_t *kyoku, *event, *detail, *counts;
} RmjLogCheckViews;
int rmj_logcheck_views(struct rmj_logcheck* c, RmjLogCheckViews* out);

/* Round boundaries and per-round score deltas for a trainer on the same GPU (what riichienv-ml's PPO worker computes on the host
 * between steps: trainers/_ppo_worker.py:100-116 GRP features, :240-266 the reward at a kyoku boundary, :283-291 rank rewards).
 * Call after every step (asynchronous on the handle's stream): d_ended [n] u8 = 0 the round goes on, 1 a round ended in this step and
 * the next one was dealt, 2 the round AND the game ended; for ended != 0, d_delta [n][4] i32 = the seats' scores now minus their
 * scores when that round was dealt, d_meta [n][4] i32 = round_wind, oya, honba, riichi_sticks at that deal (chang / ju / ben /
 * liqibang); zeros otherwise.  d_kyoku_idx [n] u8 = RiichiEnv.kyoku_idx.  Any output may be NULL.  The first call (and
 * rmj_round_track_reset) only takes the baseline; a finished game that was restarted (auto-reset / rmj_reset) re-opens without a
 * boundary.  Unlike the worker's kyoku_idx comparison a renchan counts as a boundary too (the wall's hand index moves). */
int rmj_round_track_device(rmj_handle h, uint8_t* d_ended, int32_t* d_delta, int32_t* d_meta, uint8_t* d_kyoku_idx);
int rmj_round_track_reset(rmj_handle h);
/* scores() (env.rs:401-404) into a device buffer [n][4]; d_event_counts [n] may be NULL */
int rmj_scores_device(rmj_handle h, int32_t* d_scores, uint32_t* d_event_counts);
/* RiichiEnv.points(rule_name) (riichienv-python/src/env.rs:691-727, ranks :673-689) of every game, computed on the device in f64
 * like the reference: (score - base) / 1000 * weight + uma[rank - 1]; rule 0 = "basic", 1 = "ouza-tyoujyo", 2 = "ouza-normal"
 * (3P: "basic" only; anything else -> RMJ_ERR_ARG like the reference's ValueError).  d_points / points: [n][4] f64, 0 for the
 * fourth seat of a 3P game.  The device version is asynchronous on the handle's stream (the reward of a trainer-side loop). */
int rmj_points_device(rmj_handle h, int rule, double* d_points);
int rmj_get_points(rmj_handle h, int rule, double* points);
int rmj_sync(rmj_handle h); /* wait for the handle's stream */
/* Issue all further work of the handle on the caller's HIP stream (e.g. the stream of the policy's framework), so that
 * kernels of the library and of the policy are ordered by the stream itself and no host synchronisation is needed
 * between them (NULL = the device's default stream, which is what frameworks use unless told otherwise); own != 0 returns
 * to the handle's own stream.  Work already issued is waited for first. */
int rmj_set_stream(rmj_handle h, void* hip_stream, int own);

/* ------------------------------------------------------------------ MJAI event ingestion
 * RiichiEnv.apply_event (riichienv-python/src/env.rs:880-887) -> GameState::apply_mjai_event
 * (state/event_handler.rs:18-330, state_3p/event_handler.rs:18-362) for every game at once: events[n][3] holds one MJAI
 * event per game as binary records (a start_kyoku is START_KYOKU + two TEHAI records; type NONE = no event for that
 * game).  Tile names are mapped to ids by the caller (parser.rs:336-385 mjai_to_tid; riichienv_amd/abi.py).  Afterwards
 * the observation outputs (status, legal lists, masks, waits) describe the new state like after rmj_step.
 * Bit-exact parity is claimed for full-information streams; a masked "?" tile is mapped to tile 0 by the host mapper on
 * request, like parse_mjai_tile (event_handler.rs:8-10), which leaves the masked seats in a garbage state in both
 * implementations (only the observing seat's outputs are meaningful).  The caller-side mjai_log recording of
 * env.rs:56-72 is not reproduced (start_game clears the device log, later events are not appended).
 * RMJ_EVF_REPLAY_PASS in the first record's `pad`: the bookkeeping of the reference's log walker on top of the event
 * (KyokuStepIterator, replay/mod.rs:129-177; apply_log_action, state/event_handler.rs:391-392): a seat that was offered Ron on
 * the last discard and does not win with this event has passed (same-turn furiten, permanent in riichi), a discard ends
 * the discarder's same-turn furiten, and the tile dealt after a kan (3P: after a kita too) is a rinshan draw (is_after_kan,
 * event_handler.rs:428: a win on it whose only yaku is rinshan kaihou is offered) - what (observation, action) datasets built
 * from logs need.  reach_accepted / dora events leave the published lists untouched (the claims on a riichi declaration tile
 * are decided after reach_accepted). */
#define RMJ_EVF_REPLAY_PASS 1u
int rmj_apply_events(rmj_handle h, const RmjEvent* events /*[n][3]*/);

/* Auxiliary feature blocks of an Observation that are not part of encode() / encode_extended(); absolute seat order,
 * public information only, so one block per game serves every observing seat (NP = 4, W = 34; 3P: NP = 3, W = 27):
 *   RMJ_AUX_KAWA_OVERVIEW     out[n][NP][7][W]   Observation.encode_kawa_overview (observation/python.rs:881-925,
 *                                                observation_3p/python.rs:759-810), incl. its red-five id / column quirks
 *   RMJ_AUX_YAKU_POSSIBILITY  out[n][NP][21][2]  Observation.encode_yaku_possibility (observation/python.rs:327-455,
 *                                                observation_3p/python.rs:275-400) over yaku_checker.rs:27-412
 *   RMJ_AUX_FURITEN_RON       out[n][NP][21]     Observation.encode_furiten_ron_possibility (observation/python.rs:251-293);
 *                                                all ones: the reference never fills tsumogiri_flags (observation/mod.rs:105)
 * `out` is a host pointer (rmj_encode_aux) or a device pointer written on the handle's stream (rmj_encode_aux_device). */
enum { RMJ_AUX_KAWA_OVERVIEW = 0, RMJ_AUX_YAKU_POSSIBILITY = 1, RMJ_AUX_FURITEN_RON = 2 };
int rmj_encode_aux(rmj_handle h, int which, float* out);
int rmj_encode_aux_device(rmj_handle h, int which, float* d_out);

/* Sequence (transformer) features, observation/sequence_features.rs (4-player games only, like the reference; spec
 * docs/SEQUENCE_FEATURE_ENCODING.md), for every (game, seat): Observation.encode_seq_sparse(game_style) (:331-378),
 * encode_seq_numeric (:447-471), encode_seq_candidates (:697-813) and, per game, encode_seq_progression (:503-671).
 * Arrays are padded to fixed lengths with the reference's padding values (441; (4,276,2,2,4); (279,2,2,3)), the real
 * lengths are returned beside them.  The reference derives these features from the MJAI strings an Observation
 * carries (`events`, the seat's log since its previous observation); the device defines them over the events of the
 * CURRENT ROUND, read from the binary event ring: the progression is GameState::round_seq_progression (the snapshot
 * the reference attaches with enable_seq_caching, state/mod.rs:257-260, 2150-2161), the drawn tile, the last
 * discarder and the round-start honba / deposits / scores are those of the round.  The ring must still hold the
 * round's start_kyoku (create the handle with event_ring >= 256): otherwise n_progression[g] = 0xFFFF and the
 * round-start numbers fall back to the current ones (sequence_features.rs:490).  Seats that are not to act get no
 * candidates. */
#define RMJ_SEQ_SPARSE 25
#define RMJ_SEQ_PROG 256
#define RMJ_SEQ_CAND 64
typedef struct RmjSeqBuffers {
    uint16_t* sparse;        /* [n][4][25]     token ids, padded with 441 */
    uint8_t* n_sparse;       /* [n][4]         */
    float* numeric;          /* [n][4][12]     */
    uint16_t* progression;   /* [n][256][5]    (actor, type, moqie, liqi, from), padded with (4,276,2,2,4) */
    uint16_t* n_progression; /* [n]            */
    uint16_t* candidates;    /* [n][4][64][4]  (type, moqie, liqi, from) in legal-list order, padded with (279,2,2,3) */
    uint8_t* n_candidates;   /* [n][4]         */
} RmjSeqBuffers;
/* The same features over the events of ONE OBSERVATION, as the reference's live environment computes them
 * (Observation.events = the seat's log since its previous observation, state/mod.rs:211-218; enable_seq_caching is off
 * outside the replay path): the progression holds only that delta (per seat), the drawn-tile token exists only while the
 * delta still contains the seat's tsumo, the round-start numbers come from a start_kyoku inside the delta (else the current
 * ones, sequence_features.rs:490), the last discarder is searched in the delta.  The library keeps the seats' event
 * cursors in the record: every publication of observations for an acting seat (reset, step) advances that seat's cursor
 * like get_observation does.  Seats that are not to act get empty outputs; n_progression = 0xFFFF if the ring no longer
 * holds the delta. */
#define RMJ_SEQ_DELTA_PROG 64
typedef struct RmjSeqDeltaBuffers {
    uint16_t* sparse;        /* [n][4][25]     */
    uint8_t* n_sparse;       /* [n][4]         */
    float* numeric;          /* [n][4][12]     */
    uint16_t* progression;   /* [n][4][64][5]  per seat: the delta's entries, padded with (4,276,2,2,4) */
    uint16_t* n_progression; /* [n][4]         */
    uint16_t* candidates;    /* [n][4][64][4]  */
    uint8_t* n_candidates;   /* [n][4]         */
} RmjSeqDeltaBuffers;
int rmj_encode_seq_delta(rmj_handle h, int game_style, const RmjSeqDeltaBuffers* out);          /* host arrays */
int rmj_encode_seq_delta_device(rmj_handle h, int game_style, const RmjSeqDeltaBuffers* d_out); /* device arrays, handle's stream */
int rmj_encode_seq(rmj_handle h, int game_style, const RmjSeqBuffers* out);          /* host arrays */
int rmj_encode_seq_device(rmj_handle h, int game_style, const RmjSeqBuffers* d_out); /* device arrays, handle's stream */

/* ------------------------------------------------------------------ scheduling */
/* Parts (HIP streams) a multi-step device rollout of this handle is cut into, 1..8 (default 4, or RMJ_STEP_STREAMS in
 * the environment when the handle is created); see rmj_step_random. */
int rmj_set_rollout_streams(rmj_handle h, int k);

/* Measurement entry points (rmj_bench_*, rmj_time_rollout*, rmj_total_full_path) and the test-only environment hooks are declared in
 * riichi_mi355x_bench.h: they are what bench.py, the profiles and the tests use, not part of the drop-in surface. */

#ifdef __cplusplus
}
#endif
#endif /* RIICHI_MI355X_H */
