"""GPU: the play statistics of every (kyoku, seat) of a log set (rmj_logset_playstats_device, LogSet.play_stats, riichienv_amd.stats)
against the plain restatement tests/play_stats_ref.py.  Every comparison of the table is exact integer equality, through LogSet.from_logs
and LogSet.from_text, for 4P (mode 2) and 3P (mode 5).

The hand-made logs (play_stats_ref.hand_made_logs) sit at the sizes where a walk of 64 events per pass can go wrong: logs of 0, 1, 63, 64,
65, 128 and 129 events; a START_KYOKU in lane 63 and one in lane 0 of the next pass; thirty kyokus of three events inside one pass; a hora
in lane 0 whose last tile event lies in the previous pass, and one whose last tile event lies two passes back behind 64 dora events; a
double ron and a triple hora; a reach whose discard is ronned; two reach events of one seat; a chankan after a kakan; a hora with no tile
event before it; a hora after its own dahai; events before the first START_KYOKU; events with actor 4 and 5; 3P: kita and an event of
seat 3."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from riichienv_amd import abi, datasets, grp, stats, vecenv
from riichienv_amd.logset import LogSet
from tests import grp_ref
from tests import play_stats_ref as R

pytestmark = pytest.mark.gpu
MODES = [(4, 2), (3, 5)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GAMES = {}


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def _text(logs):
    return [("\n".join(json.dumps(ev) for ev in log) + "\n").encode() for log in logs]


def _sets(logs, n, **kw):
    """the same logs as a set packed from dicts and as a set parsed from text"""
    return {"from_logs": LogSet.from_logs(logs, num_players=n), "from_text": LogSet.from_text(_text(logs), num_players=n, **kw)}


def _assert_table(ls, want, koff, what):
    got = ls.play_stats()
    rows = got["rows"].cpu().numpy()
    assert rows.dtype == np.int32 and rows.shape == want.shape, (what, rows.shape, want.shape)
    bad = np.argwhere(rows != want)
    assert not len(bad), (what, len(bad), [(b.tolist(), int(rows[tuple(b)]), int(want[tuple(b)])) for b in bad[:6]])
    assert got["kyoku_offsets"].cpu().tolist() == list(koff), what
    assert got["log_of"].cpu().tolist() == np.repeat(np.arange(len(koff) - 1), np.diff(koff)).tolist(), what
    return got


@pytest.mark.parametrize("seats,mode", MODES)
def test_hand_made_logs(seats, mode):
    named = R.hand_made_logs(seats)
    logs = list(named.values())
    want, koff = R.table(logs, seats), R.kyoku_offsets(logs)
    assert koff[1] == 0 and want.shape[0] > 40
    for what, ls in _sets(logs, seats).items():
        got = _assert_table(ls, want, koff, what)
        assert bool(got["valid"].all())
        ls.close()
    # every log alone: the walk starts at event 0 of the stream
    for name, log in named.items():
        if len(log) in (0, 65, 129) or name in ("hora_lane0", "sk_lane63_lane0"):
            for what, ls in _sets([log], seats).items():
                _assert_table(ls, R.kyoku_rows(log, seats), R.kyoku_offsets([log]), (name, what))
                ls.close()
    # the holders forward
    for src in (datasets.LogSampleBuilder.from_text(_text(logs), game_mode=mode), grp.GrpDataset.from_text(_text(logs), game_mode=mode)):
        assert np.array_equal(src.play_stats()["rows"].cpu().numpy(), want) and np.array_equal(stats.play_stats(src)["rows"].cpu().numpy(), want)
        src.close()


@pytest.mark.parametrize("seats,mode", MODES)
def test_event_soup_between_guard_words(seats, mode):
    torch, dev = _torch()
    L = vecenv.load_lib()
    logs = R.soup_logs(400, seats, 1000 + seats)
    want, koff = R.table(logs, seats), R.kyoku_offsets(logs)
    K, G = want.shape[0], 64
    assert K > 2000 and want[:, :, R.DEAL_IN].sum() > 50 and want[:, :, R.WIN_TSUMO].sum() > 10 and want[:, :, R.RIICHI_TURN].max() >= 2 and want[:, :, R.WIN_TURN].max() >= 1
    for what, ls in _sets(logs, seats).items():
        _assert_table(ls, want, koff, what)
        buf = torch.full((G + K * 64 + G,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        ptr = buf.data_ptr() + G * 4
        for fill in ("sentinel", "garbage"):
            if fill == "garbage":
                buf[G: G + K * 64] = torch.randint(-2 ** 31, 2 ** 31 - 1, (K * 64,), dtype=torch.int64, device=dev).to(torch.int32)
            assert L.rmj_logset_playstats_device(ls.handle, seats, C.c_void_p(ptr), None) == 0
            torch.cuda.synchronize()
            h = buf.cpu().numpy()
            assert (h[:G] == 0x5A5A5A5A).all() and (h[G + K * 64:] == 0x5A5A5A5A).all(), (what, fill)
            assert np.array_equal(h[G: G + K * 64].reshape(K, 4, 16), want), (what, fill)
        ls.close()


def test_golden_log_alone_and_among_copies_in_reverse_order():
    with open(os.path.join(ROOT, "tests", "golden", "126_204_0_mjai.jsonl"), "rb") as f:
        raw = f.read()
    log = [json.loads(l) for l in raw.split(b"\n") if l.strip()]
    want = R.kyoku_rows(log, 4)
    assert want.shape[0] == 12 and R.derived_horas(log, 4) == R.target_horas(log, 4)
    for what, ls in _sets([log], 4).items():
        _assert_table(ls, want, [0, 12], what)
        ls.close()
    if not raw.endswith(b"\n"):
        raw += b"\n"
    ends = np.arange(1, 65) * len(raw)
    ranges = np.stack([ends - len(raw), ends], axis=1)[::-1].copy()
    for what, ls in {"ranges": LogSet.from_text(raw * 64, ranges=ranges, num_players=4), "dicts": LogSet.from_logs([log] * 64, num_players=4)}.items():
        got = _assert_table(ls, np.concatenate([want] * 64), np.arange(65) * 12, what)
        assert np.array_equal(got["rows"][37 * 12: 38 * 12].cpu().numpy(), want)
        ls.close()


def _games(mode, n=16):
    """n device-played games of `mode` under step_greedy until done: (text uint8 and offsets int64 on the device, the logs as dicts)"""
    if mode not in _GAMES:
        from riichienv_amd.torch_env import TorchVecEnv

        tenv = TorchVecEnv(n, game_mode=mode, seed=91 + mode, skip_mjai_logging=False, event_ring=8192)
        env = tenv.env
        env.reset()
        for _ in range(40):
            env.step_greedy(7, 500, auto_reset=False, call_rate_256=64)
            if env.status()[2].all():
                break
        assert env.status()[2].all() and int(env.events_lost().sum()) == 0
        text, offs = tenv.drain_text(cursor=env.log_positions()[0].copy(), peek=True)
        text, offs = text.clone(), offs.clone()
        raw, o = text.cpu().numpy().tobytes(), offs.cpu().tolist()
        logs = [[json.loads(l) for l in raw[o[g]: o[g + 1]].split(b"\n") if l.strip()] for g in range(n)]
        env.close()
        _GAMES[mode] = (text, offs, logs)
    return _GAMES[mode]


def _same_summary(got, want, what):
    assert list(got) == list(want), (what, list(got), list(want))
    for k in want:
        for a, b in zip(got[k] if isinstance(got[k], list) else [got[k]], want[k] if isinstance(want[k], list) else [want[k]]):
            assert (math.isnan(a) and math.isnan(b)) or a == b, (what, k, got[k], want[k])


@pytest.mark.parametrize("seats,mode", MODES)
def test_self_written_logs_and_their_summary(seats, mode):
    text, offs, logs = _games(mode)
    want, koff = R.table(logs, seats), R.kyoku_offsets(logs)
    # a condition on the input: the corpus holds every kind of round end and play the columns tell apart
    assert want[:, :, R.DEAL_IN].sum() >= 1 and want[:, :, R.WIN_TSUMO].sum() >= 1 and want[:, :, R.RIICHI_ACCEPTED].sum() >= 1 and want[:, :, R.CALLS].sum() >= 1
    assert ((want[:, 0, R.END] & 2) != 0).any() and (seats == 4 or want[:, :, R.KITA].sum() >= 1)
    for log in logs:
        assert R.derived_horas(log, seats) == R.target_horas(log, seats)
    ls = LogSet.from_device_text(text, offs, num_players=seats)
    _assert_table(ls, want, koff, "device text")
    # summarize on the device table against the summary of the restatement's table, key for key
    ref = grp_ref.logset_rows(logs, seats)
    table = {"rows": want, "valid": np.ones(len(want), bool), "log_of": np.repeat(np.arange(len(logs)), np.diff(koff)), "num_players": seats,
             "start_scores": ls.start_scores, "end_scores": ls.end_scores, "rank": ref["rank"]}
    hero = np.random.default_rng(5).integers(0, seats, len(logs))
    for h in (None, hero):
        got = stats.summarize(ls, hero=h)
        _same_summary(got, stats.summarize(table, hero=h), ("hero", h is not None))
        assert got["kyokus"] == len(want) * (seats if h is None else 1) and 0 < got["win_rate"] < 1 and got["rank_rates"] and abs(sum(got["rank_rates"]) - 1) < 1e-12
        assert got["win_points_mean"] > 0 and (h is not None or got["deal_in_points_mean"] > 0)
    _same_summary(stats.summarize(ls, hero=hero, table=ls.play_stats()), stats.summarize(table, hero=hero), "a table built before")
    assert np.array_equal(ls.final_ranks().cpu().numpy(), ref["rank"])
    _same_summary(stats.summarize(ls.play_stats()), stats.summarize({k: v for k, v in table.items() if k not in ("start_scores", "end_scores", "rank")}), "table dict")
    ls.close()
    ld = LogSet.from_logs(logs, num_players=seats)
    _assert_table(ld, want, koff, "dicts")
    _same_summary(stats.summarize(ld, hero=hero), stats.summarize(table, hero=hero), "dict set")
    ld.close()


@pytest.mark.parametrize("seats,mode", MODES)
def test_on_error_keep_marks_the_rows_of_broken_logs(seats, mode):
    logs = list(R.hand_made_logs(seats).values()) + R.soup_logs(40, seats, 77) + _games(mode)[2][:4]
    texts = _text(logs)
    broken = [5, len(logs) - 2]                                    # a hand-made log and a whole game
    for i in broken:
        assert R.kyoku_offsets(logs)[i + 1] > R.kyoku_offsets(logs)[i]
        lines = texts[i].split(b"\n")
        lines[1] = lines[1][: len(lines[1]) // 2]                  # half a JSON object
        texts[i] = b"\n".join(lines)
    with pytest.raises(ValueError):
        LogSet.from_text(texts, num_players=seats)
    ls = LogSet.from_text(texts, num_players=seats, on_error="keep")
    assert [d[0] for d in ls.dropped] == broken
    # the rows of a broken log are -1 whatever its records hold; its kyoku count is the parser's
    koff = ls.kyoku_offsets.astype(np.int64)
    good = [i for i in range(len(logs)) if i not in broken]
    assert all(koff[i + 1] - koff[i] == len(R.kyoku_rows(logs[i], seats)) for i in good)
    want = np.concatenate([R.kyoku_rows(logs[i], seats) if i in good else np.full((koff[i + 1] - koff[i], 4, 16), -1, np.int32) for i in range(len(logs))])
    got = _assert_table(ls, want, koff, "keep")
    valid = got["valid"].cpu().numpy()
    assert valid.dtype == bool and np.array_equal(valid, ~np.isin(got["log_of"].cpu().numpy(), broken)) and np.array_equal(valid, want[:, 0, 0] >= 0)
    alone = LogSet.from_text([texts[i] for i in good], num_players=seats)
    hero_all = np.random.default_rng(9).integers(0, seats, len(logs))
    _same_summary(stats.summarize(ls), stats.summarize(alone), "keep against the good logs alone")
    _same_summary(stats.summarize(ls, hero=hero_all), stats.summarize(alone, hero=hero_all[good]), "keep, hero")
    ls.close()
    alone.close()


def test_refused_arguments():
    torch, dev = _torch()
    L = vecenv.load_lib()
    ls = LogSet.from_logs(list(R.hand_made_logs(4).values()), num_players=4)
    rows = torch.zeros((ls.n_kyokus + 1, 4, 16), dtype=torch.int32, device=dev)
    p = rows.data_ptr()
    assert L.rmj_logset_playstats_device(None, 4, C.c_void_p(p), None) == -1
    assert L.rmj_logset_playstats_device(ls.handle, 4, None, None) == -1
    assert L.rmj_logset_playstats_device(ls.handle, 5, C.c_void_p(p), None) == -1
    assert L.rmj_logset_playstats_device(ls.handle, 2, C.c_void_p(p), None) == -1
    assert L.rmj_logset_playstats_device(ls.handle, 4, C.c_void_p(p + 4), None) == -1
    torch.cuda.synchronize()
    assert not bool(rows.any())                                      # a refused call writes nothing
    assert L.rmj_logset_playstats_device(ls.handle, 4, C.c_void_p(p), None) == 0
    with pytest.raises(ValueError):
        ls.play_stats(num_players=5)
    ls.close()
    with pytest.raises(vecenv.RmjError):
        ls.play_stats()
    empty = LogSet.from_logs([[{"type": "start_game"}, {"type": "end_game"}], []], num_players=4)     # a set without a kyoku
    assert empty.n_kyokus == 0 and L.rmj_logset_playstats_device(empty.handle, 4, C.c_void_p(p), None) == 0
    assert tuple(empty.play_stats()["rows"].shape) == (0, 4, 16) and stats.summarize(empty)["kyokus"] == 0.0
    empty.close()
    with pytest.raises(TypeError):
        stats.play_stats(object())


def test_the_example_runs():
    """examples/play_stats.py: two greedy rollouts -> drain_text -> LogSet.from_device_text -> summarize, side by side"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "play_stats.py"), "--games", "8", "--steps", "20000"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "call_rate" in p.stdout and "win_rate" in p.stdout and "deal_in_rate" in p.stdout
