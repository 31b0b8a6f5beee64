"""Stream order and pointer passing between torch and the library, in one place ("Torch-side calls").

A handle either shares torch's stream (rmj_set_stream: torch's stream orders the library's kernels with torch's own, nothing waits on
the host) or keeps the library's own hipStreamNonBlocking stream, which nothing orders against torch's.  In own-stream mode every call
therefore waits for torch's current stream first - the tensors it is handed, or writes, were made there - and for the library's stream
afterwards.  StreamLink.call is that rule; torch is used for streams and device memory only."""
from __future__ import annotations

from . import abi, vecenv


def stream_ptr(torch, device):
    """torch's current stream of `device` as the integer the stream-argument entries take (rmj_logset_grp_device,
    rmj_logset_playstats_device, rmj_grp_rows_device)"""
    return torch.cuda.current_stream(device).cuda_stream


class StreamLink:
    """link = StreamLink(torch, device, env, shared); link.call(L.rmj_scores_device, env.h, scores, None)

    env: the VecRiichiEnv whose handle's stream the link speaks for (collectors and builders made over that environment call with their
    own handles: the caller passes the handle).  shared: the handle issues on torch's stream (after bind).  owner: what the tensors of
    wrap() keep alive (default: env)."""

    def __init__(self, torch, device, env, shared=False, owner=None):
        self.torch, self.device, self.env, self.shared = torch, device, env, bool(shared)
        self.owner = env if owner is None else owner

    def bind(self, stream=None):
        """rmj_set_stream: the handle's further work is issued on `stream` (a torch.cuda.Stream; default: torch's current stream of the
        device); work already issued is waited for first.  Returns the stream."""
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        vecenv._chk(self.env.L.rmj_set_stream(self.env.h, s.cuda_stream, 0))
        self.shared = True
        return s

    def stream_ptr(self):
        return stream_ptr(self.torch, self.device)

    def wrap(self, ptr, shape, typestr, owner=None):
        """a zero-copy tensor over library-owned device memory (abi.device_tensor)"""
        return abi.device_tensor(self.torch, self.owner if owner is None else owner, self.device, ptr, shape, typestr)

    def _ptr(self, a):
        if not hasattr(a, "data_ptr"):
            return a
        if a.device != self.device or not a.is_contiguous():
            raise ValueError(f"the library takes contiguous tensors on {self.device} (got one on {a.device}, contiguous: {a.is_contiguous()})")
        return a.data_ptr()

    def call(self, fn, *args):
        """fn(*args) with every torch tensor passed as its device pointer (None and everything else as it is); a non-zero return code
        raises RmjError.  Shared stream: nothing else - no allocation, no synchronisation, so the call can be captured in a HIP graph.
        Own stream: torch's current stream is waited for before the call and the library's stream after it."""
        args = [self._ptr(a) for a in args]
        if not self.shared:
            self.torch.cuda.current_stream(self.device).synchronize()
        vecenv._chk(fn(*args))
        if not self.shared:
            self.env.sync()
