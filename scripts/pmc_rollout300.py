#!/usr/bin/env python3
"""The launch shape of profiles/r06_pmc_k_step4.json and profiles/turn_end_shared.json for a counter pass: 65 536 4p-red-half games, one
6 000-step fused RandomAgent launch to leave the synchronised start behind, then three launches of 300 steps (k_step4_queue<0>).

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_BRANCH --output-format csv -d OUT -- python3 scripts/pmc_rollout300.py

(counters in a run of their own, no tracing beside them; RMJ_LIB_PATH selects another build of the library)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from riichienv_amd import vecenv  # noqa: E402

env = vecenv.VecRiichiEnv(65536, game_mode=2, seed=0)
env.reset()
env.step_random(0xC0FFEE, 6000, auto_reset=True)
env.total_steps()
for _ in range(3):
    env.step_random(0xC0FFEE, 300, auto_reset=True)
    env.total_steps()
env.close()
