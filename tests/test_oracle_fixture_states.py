"""The reference's agari fixtures (tests/golden/agari_{4p,3p}.json) as game states (tests/fixture_states.py), settled by the oracle's
state machine: the discard before the win offers it to the winner alone, the greedy policy takes it, the win ends the game and
win_results gives the fixture's is_win, han, fu and yaku in order.  This pins the state builder that
tests/test_gpu_fixture_settlement.py runs through every step path."""
import collections

import pytest

from riichienv_amd.abi import RON, TSUMO, WAIT_ACT, WAIT_RESPONSE, unpack_action
from tests import fixture_states as fs

# fixtures whose Conditions the state machine cannot reproduce exactly (FixtureState.excluded): compared with the oracle only
EXCLUDED = {"agari_4p.json": 0, "agari_3p.json": 0}


@pytest.mark.parametrize("name", list(fs.FILES))
def test_fixture_states_settle_to_the_fixture(name):
    np_ = fs.FILES[name]
    cases = fs.load(name)
    excluded = collections.Counter()
    for i, c in enumerate(cases):
        for rep in range(2):
            st, g = fs.build_case(c, np_, **fs.replica(i, rep, np_))   # (g: the builder's game, one step on: the discard is made)
            want = TSUMO if c["conditions"]["tsumo"] else RON
            assert g.status()[:2] == (1 << st.winner, WAIT_ACT if want == TSUMO else WAIT_RESPONSE), (name, i, rep, g.status())
            assert unpack_action(st.action)[0] == want and st.action in g.legal(st.winner), (name, i, rep)
            assert g.greedy_actions(fs.PSEED, i, fs.CALL_RATE)[st.winner] == st.action, (name, i, rep)
            g.step({st.winner: st.action})
            assert g.status()[2] == 1, (name, i, rep, "the win does not end the game")
            w = g.win_results()[st.winner]
            if st.excluded:
                excluded[st.excluded] += rep == 0
                continue
            e = c["expected"]
            assert (w["is_win"], w["han"], w["fu"], w["yaku"]) == (e["is_win"], e["han"], e["fu"], e["yaku"]), (name, i, rep, w, e)
    assert sum(excluded.values()) == EXCLUDED[name], dict(excluded)
