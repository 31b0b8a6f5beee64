"""CPU: what the log classes (logset.LogSet, datasets.LogSampleBuilder, grp.GrpDataset) decide before any library call, through every
public constructor: the argument errors and their messages.  No constructor here gets as far as the device."""
import os
import re

import pytest

from riichienv_amd import abi, replay
from riichienv_amd.datasets import LogSampleBuilder
from riichienv_amd.grp import GrpDataset
from riichienv_amd.logset import LogSet

LOG = os.path.join(os.path.dirname(__file__), "golden", "126_204_0_mjai.jsonl")
TEXT = [b'{"type":"start_game"}\n']


def _text_constructors(cls):
    """(name, call(**kw)) of the constructors that take text; the device one is given no tensors: it must not get to look at them"""
    return [("from_text", lambda **kw: cls.from_text(TEXT, **kw)), ("from_jsonl", lambda **kw: cls.from_jsonl([LOG], **kw)),
            ("from_device_text", lambda **kw: cls.from_device_text(None, None, **kw))]


def _constructors(cls):
    """every public constructor; the dict ones over no logs, from_logset over the empty set (neither makes a library call)"""
    return [("dicts", lambda **kw: cls([], **kw)), ("from_logset", lambda **kw: cls.from_logset(LogSet.from_logs([]), **kw))] + _text_constructors(cls)


def _raises(call, exc, message, **kw):
    with pytest.raises(exc, match=re.escape(message)):
        call(**kw)


def test_on_error_outside_the_allowed_set():
    for _, call in _text_constructors(LogSet):
        _raises(call, ValueError, "on_error is 'raise', 'drop' or 'keep'", on_error="ignore")
    for cls in (LogSampleBuilder, GrpDataset):
        for _, call in _text_constructors(cls):
            _raises(call, ValueError, "on_error is 'raise' or 'drop'", on_error="ignore")
            _raises(call, ValueError, "on_error is 'raise' or 'drop'", on_error="keep")


def test_unknown_features_and_rule():
    for _, call in _constructors(LogSampleBuilder):
        _raises(call, ValueError, f"unknown feature set 'nope': one of {sorted(abi.FEATURES)}", features="nope")
        _raises(call, ValueError, "Unknown rule: 'other'. Expected 'tenhou' or 'mjsoul'", rule="other")


def test_a_range_ending_behind_the_text():
    for cls in (LogSet, LogSampleBuilder, GrpDataset):
        _raises(lambda **kw: cls.from_text(b"{}\n", ranges=[[0, 9]], **kw), ValueError, "a range ends behind the text")
        _raises(lambda **kw: cls.from_text(b"{}\n{}\n", ranges=[[3, 6], [0, 7]], **kw), ValueError, "a range ends behind the text", on_error="drop")


def test_n_slots_and_capacity():
    events = replay.load_mjai_jsonl(LOG)
    for n in (0, 2, -1):
        _raises(lambda **kw: LogSampleBuilder([events], **kw), ValueError, "n_slots must be between 1 and the number of logs (1)", n_slots=n)
    _raises(lambda **kw: LogSampleBuilder([], **kw), ValueError, "n_slots must be between 1 and the number of logs (0)", n_slots=1)
    _raises(lambda **kw: LogSampleBuilder.from_logset(LogSet.from_logs([]), **kw), ValueError, "n_slots must be between 1 and the number of logs (0)", n_slots=1)
    for _, call in _constructors(LogSampleBuilder):
        for c in (0, -5):
            _raises(call, ValueError, "capacity must be positive (samples)", capacity=c)


def test_grp_dataset_keywords():
    for _, call in _constructors(GrpDataset):
        _raises(call, TypeError, "unexpected arguments ['no_such_argument']", no_such_argument=1)
        _raises(call, TypeError, "unexpected arguments ['on_errors']", features="base", on_errors="drop")
    for _, call in _constructors(LogSampleBuilder):
        with pytest.raises(TypeError):
            call(no_such_argument=1)


def test_the_empty_sets_need_no_device():
    s = LogSet.from_logs([])
    assert (s.M, s.n_events, s.n_kyokus, s.longest_log, s.handle, s.owns_tables) == (0, 0, 0, 0, None, False)
    assert s.kyoku_offsets.tolist() == [0] and s.lengths.tolist() == [] and s.decisions.tolist() == [] and s.start_scores.shape == (0, 4)
    b = LogSampleBuilder.from_logset(s, n_slots=0)
    assert (b.M, b.n_slots, b.capacity, b.run()) == (0, 0, 64, 0) and b.logset is s
    d = GrpDataset.from_logset(s, gamma=0.5)
    assert d.M == 0 and d.n_kyokus == 0 and d.logset is s
    b.close()
    d.close()
    s.close()
    s.close()
