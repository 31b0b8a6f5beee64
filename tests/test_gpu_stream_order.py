"""Own-stream mode (share_stream=False) while torch's stream is BUSY: the library's stream is ordered against nothing, so every call
has to wait for torch's stream first (streams.StreamLink.call) - the tensors it writes were allocated and filled there, and a fill that
lands after the library's kernel wipes its result.  A quiet stream hides that; here each call under test is issued with work still
running on torch's current stream, and its result is held to a share_stream=True twin of the same seed."""
import gc
import time

import pytest

pytestmark = pytest.mark.gpu

N, SEED = 64, 4242
# torch.cuda._sleep(BUSY_CYCLES) keeps the stream busy for 41.9 ms on an MI355X (HIP events: 4.2 ms per 10 ** 7 cycles), and
# constructing a 64-game own-stream TorchVecEnv behind it takes 0.6-1.2 ms of host time (profiles/stream_link.json), so the work is
# still running when the call under test is made - unless the runtime puts the new environment's stream on the hardware queue of the
# busy stream (it deals streams out to a few queues: the fourth construction behind a sleep measured 42.2 ms, the sleep's length, on
# the parent commit as well), in which case the reset kernel of the constructor has queued behind the sleep; the construction is then
# repeated with that environment kept alive, so that the next stream goes to another queue.  The guard below is asserted on what the
# last attempt left.  On the parent commit obs, scores and sample_ids fail their comparison; round_track and points pass there too.
BUSY_CYCLES = 10 ** 8
ATTEMPTS = 4
CALLS = ("obs", "scores", "sample_ids", "round_track", "points")


def _results(env, call):
    """the tensors one call under test returns, as a tuple"""
    if call == "obs":
        return (env.obs(),)
    if call == "scores":
        return (env.scores(),)
    if call == "sample_ids":
        return (env.sample_ids(None, 11),)
    if call == "round_track":
        return tuple(env.round_track())
    return (env.points(),)


@pytest.fixture(scope="module")
def twins():
    """(side stream, {mode: {call: results}} of the shared-stream twin), computed once per mode (no call steps a game: the order does
    not matter); one own-stream environment is made and used on the side stream first, so that no test pays a first-use cost"""
    torch = pytest.importorskip("torch")
    from riichienv_amd.torch_env import TorchVecEnv

    out = {}
    for mode in (2, 5):
        env = TorchVecEnv(N, game_mode=mode, seed=SEED, share_stream=True)
        out[mode] = {call: tuple(x.clone() for x in _results(env, call)) for call in CALLS}
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(10 ** 6)
        env = TorchVecEnv(N, game_mode=2, seed=SEED, share_stream=False)
        for call in CALLS:
            _results(env, call)
    del env
    torch.cuda.synchronize()
    return side, out


@pytest.mark.parametrize("mode", [2, 5])
@pytest.mark.parametrize("call", CALLS)
def test_first_call_on_a_busy_stream_matches_the_shared_twin(twins, mode, call):
    torch = pytest.importorskip("torch")
    from riichienv_amd.torch_env import TorchVecEnv

    side, want = twins[0], twins[1][mode][call]
    gc.collect()      # an environment of an earlier test that is freed during this one waits for the whole device, the busy work included
    ev, held = torch.cuda.Event(), []
    with torch.cuda.stream(side):
        if call in ("obs", "scores"):                        # their tensors are zero-filled by the constructor; the others' by the first call
            for attempt in range(ATTEMPTS):
                torch.cuda._sleep(BUSY_CYCLES)
                ev.record()
                t0 = time.perf_counter()
                env = TorchVecEnv(N, game_mode=mode, seed=SEED, share_stream=False)
                if not ev.query() or attempt == ATTEMPTS - 1:
                    break
                held.append(env)                             # kept alive: its stream stays on the side stream's hardware queue, the next goes elsewhere
        else:
            env = TorchVecEnv(N, game_mode=mode, seed=SEED, share_stream=False)
            side.synchronize()
            torch.cuda._sleep(BUSY_CYCLES)
            ev.record()
            t0 = time.perf_counter()
        print(f"{call}-{mode}: host ms from the event to the call: {(time.perf_counter() - t0) * 1e3:.3f}")
        assert not ev.query(), "the busy work ended before the call under test: it proves nothing"
        got = _results(env, call)
        assert not env.shared and len(got) == len(want)
        for i, (x, w) in enumerate(zip(got, want)):
            assert torch.equal(x, w), (call, i)              # (read on the side stream: behind whatever was still queued there)
    side.synchronize()
