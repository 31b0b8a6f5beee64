"""StreamLink (riichienv_amd/streams.py), the one owner of stream order and pointer passing on the torch side, against stand-ins that
log what happens: no GPU, no torch, no library."""
import ctypes as C

import pytest

from riichienv_amd import vecenv
from riichienv_amd.streams import StreamLink, stream_ptr

DEV, OTHER = "cuda:0", "cuda:1"


class FakeStream:
    cuda_stream = 0x5EED

    def __init__(self, log):
        self.log = log

    def synchronize(self):
        self.log.append("torch wait")


class FakeTorch:
    """torch.cuda.current_stream(device) and nothing else"""

    def __init__(self, log):
        self.cuda, self._stream = self, FakeStream(log)

    def current_stream(self, device):
        assert device == DEV
        return self._stream


class FakeTensor:
    def __init__(self, ptr, device=DEV, contiguous=True):
        self.ptr, self.device, self.contiguous = ptr, device, contiguous

    def data_ptr(self):
        return self.ptr

    def is_contiguous(self):
        return self.contiguous


class FakeLib:
    """entries that log themselves with the arguments they were given"""

    def __init__(self, log):
        self.log, self.rc = log, 0

    def rmj_entry(self, *args):
        self.log.append(("entry",) + args)
        return self.rc

    def rmj_sync(self, h):
        self.log.append(("rmj_sync", h))
        return 0

    def rmj_set_stream(self, h, stream, flags):
        self.log.append(("rmj_set_stream", h, stream, flags))
        return 0

    def rmj_last_error(self):
        return b"made to fail"


@pytest.fixture
def rig(monkeypatch):
    log = []
    lib = FakeLib(log)
    monkeypatch.setattr(vecenv, "_LIB", lib)           # (RmjError's text comes from rmj_last_error of the loaded library)
    env = object.__new__(vecenv.VecRiichiEnv)           # a real environment object over the stand-in library: sync() is its own
    env.L, env.h = lib, "handle"
    return log, lib, StreamLink(FakeTorch(log), DEV, env)


def test_own_stream_call_is_wait_entry_sync(rig):
    log, lib, link = rig
    assert not link.shared
    link.call(lib.rmj_entry, "handle", 3)
    assert log == ["torch wait", ("entry", "handle", 3), ("rmj_sync", "handle")]


def test_shared_call_is_the_entry_alone(rig):
    log, lib, link = rig
    link.shared = True
    link.call(lib.rmj_entry, "handle", 3)
    assert log == [("entry", "handle", 3)]


def test_bind_sets_the_stream_once_and_flips_the_mode(rig):
    log, lib, link = rig
    s = link.bind()
    assert log == [("rmj_set_stream", "handle", FakeStream.cuda_stream, 0)] and link.shared and s.cuda_stream == FakeStream.cuda_stream
    other = FakeStream(log)
    other.cuda_stream = 0xBEEF
    del log[:]
    assert link.bind(other) is other
    assert log == [("rmj_set_stream", "handle", 0xBEEF, 0)] and link.shared
    link.call(lib.rmj_entry, "handle")
    assert log[1:] == [("entry", "handle")]


def test_stream_ptr_is_the_current_streams_integer(rig):
    log, _lib, link = rig
    assert link.stream_ptr() == stream_ptr(link.torch, DEV) == FakeStream.cuda_stream and log == []


@pytest.mark.parametrize("shared", [False, True])
def test_tensors_arrive_as_pointers_none_as_none(rig, shared):
    log, lib, link = rig
    link.shared = shared
    ref = C.byref(C.c_uint32())
    link.call(lib.rmj_entry, "other handle", FakeTensor(0x1000), None, 7, ref, FakeTensor(0x2000))
    entry = [e for e in log if e[0] == "entry"]
    assert entry == [("entry", "other handle", 0x1000, None, 7, ref, 0x2000)]


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("bad", [FakeTensor(0x1000, contiguous=False), FakeTensor(0x1000, device=OTHER)], ids=["strided", "other device"])
def test_a_strided_or_foreign_tensor_is_refused_before_the_entry(rig, shared, bad):
    log, lib, link = rig
    link.shared = shared
    with pytest.raises(ValueError):
        link.call(lib.rmj_entry, "handle", FakeTensor(0x3000), bad)
    assert log == []


@pytest.mark.parametrize("shared", [False, True])
def test_a_failing_entry_raises_and_nothing_follows_it(rig, shared):
    log, lib, link = rig
    link.shared = shared
    lib.rc = 5
    with pytest.raises(vecenv.RmjError, match="rmj error 5: made to fail"):
        link.call(lib.rmj_entry, "handle")
    assert log[-1] == ("entry", "handle") and len(log) == (1 if shared else 2)
