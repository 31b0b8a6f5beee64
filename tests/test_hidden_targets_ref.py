"""The yardstick of the hidden-hand targets (tests/hidden_targets_ref.py) on hand-made states: no GPU."""
import pytest

from oracle import oracle
from tests import apply_events_util as U
from tests import hidden_targets_ref as H

M2, M3 = 1 << 1, 1 << 2   # 2m, 3m as wait bits


def _state_before_ryukyoku(log):
    """the oracle's state once every event in front of the log's ryukyoku is applied (replay mode), and that event's index"""
    game = oracle.Game(game_mode=2, skip_log=True)
    for i, ev in enumerate(log):
        if ev["type"] == "ryukyoku":
            return game.peek(), i
        game.apply_event(ev, replay=True)
    raise AssertionError("no ryukyoku")


def test_the_furiten_hand_is_tenpai_on_2m_3m():
    game = oracle.Game(game_mode=2, skip_log=True)
    for ev in U.furiten_log(False)[:2]:
        game.apply_event(ev, replay=True)
    hist, sh, waits, flags = H.seat_fields(game.peek().players[1], False)
    assert hist.sum() == 13 and hist[0] == 3 and hist[1] == 1 and hist[18:27].tolist() == [1] * 9
    assert sh == 0 and waits == M2 | M3
    assert flags == H.PRESENT | H.TENPAI   # closed, no riichi, nothing discarded yet


@pytest.mark.parametrize("riichi", [False, True])
def test_missed_win_furiten_shows_on_seat_1_as_an_opponent(riichi):
    view, at = _state_before_ryukyoku(U.furiten_log(riichi))
    assert at == (20 if riichi else 10)   # the flags are set by the events up to 19 / 9
    p = view.players[1]
    assert (bool(p.missed_agari_riichi), bool(p.missed_agari_doujun)) == (riichi, not riichi)
    assert not any(int(d) >> 2 in (1, 2) for d in p.discards[: p.n_discards]), "furiten must come from the missed win, not from the seat's own discards"
    want = H.PRESENT | H.TENPAI | H.FURITEN | (H.RIICHI if riichi else 0)
    for hero, r in ((0, 0), (3, 1), (2, 2)):   # seat 1 is shimocha of 0, toimen of 3, kamicha of 2
        row = H.targets_of_view(view, hero, 4)
        assert int(row["opp_flags"][r]) == want, (hero, r)
        assert int(row["opp_waits"][r]) == M2 | M3 and int(row["opp_shanten"][r]) == 0
        assert int(row["opp_hand"][r].sum()) == 13


def test_rows_of_seats_that_do_not_exist_are_zero():
    game = oracle.Game(game_mode=5, skip_log=True)
    game.reset()
    view = game.peek()
    row = H.targets_of_view(view, 0, 3)
    assert row["opp_flags"].tolist()[:2] == [row["opp_flags"][0]] * 2 and row["opp_flags"][0] & H.PRESENT
    assert row["opp_flags"][2] == 0 and not row["opp_hand"][2].any() and row["opp_waits"][2] == 0 and row["opp_shanten"][2] == 0
    none = H.targets_of_view(view, 3, 3)
    assert not any(none[f].any() for f in H.FIELDS)


def test_log_targets_covers_every_seat_at_every_event():
    log = U.furiten_log(True)
    rows = H.log_targets(log, 2)
    assert set(rows) == {(i, s) for i in range(len(log)) for s in range(4)}
    some = H.log_targets(log, 2, keys={(20, 0), (3, 2)})
    assert set(some) == {(20, 0), (3, 2)}
    for k, row in some.items():
        assert all((row[f] == rows[k][f]).all() for f in H.FIELDS)
    assert int(rows[20, 0]["opp_flags"][0]) & H.FURITEN and not int(rows[2, 0]["opp_flags"][0]) & H.FURITEN
