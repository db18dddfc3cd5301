"""Where and when the library's work runs: the stream, thread and device contract at the head of include/xparcel.h, held for
every entry point that takes a stream through the recipes of tests/stream_cases.py (what the kernels compute is the business
of the other device tests).  Every comparison is bit for bit -- dtype, shape and np.array_equal(equal_nan=True) -- against the
same recipe run on synchronised inputs on the default stream: the kernels are deterministic (their only atomics are integer
tile counters), so there is no tolerance here and none may be introduced.

(a) test_side_stream: the inputs are NaN-filled buffers (integers and masks zero); on a fresh side stream a delay is enqueued,
    then the copies of the real inputs into the buffers, then the recipe.  The event behind the delay must still be pending
    when the recipe returns (the call did not block, and the delay covered the whole enqueue); after the stream has drained
    the outputs equal the reference.  Whatever the call puts on another stream runs ahead of the delayed copies, reads NaN
    (valid memory, legal input) and gives a wrong answer, never a fault.
(b) test_host_buffers_on_a_side_stream: NumPy inputs with _Call.run patched to pass a side stream's handle where it passes
    NULL; the outputs are compared the moment the call returns, behind a delay on that stream.
(c) test_four_threads_four_streams, test_persistent_kernels_on_two_streams: concurrent callers.
(d) test_last_error_is_thread_local.  (e) test_another_current_device.  (f) test_side_stream_reached_every_entry_point.

The delay is torch.cuda._sleep, calibrated once per session with events, in a ladder of three (DELAYS_MS): the first rung
whose event is still pending when the recipe returns counts; if none is, the test fails with "delay too short".
Measured on an MI355X, the host time of enqueuing a recipe on the side stream (float32 and float64 alike): the single calls
0.06 ... 0.4 ms (crossing_level 0.06, cape_surface_family 0.24, cape_densify 0.39); the chains ecape 0.44, corfidi_storm_motion
0.43, effective_layer_chain 0.50, conv_properties_and_proxies 0.65 ms; the two persistent grids,
where allocating the outputs dominates, persistent_fused 3.7 and persistent_surface 5.4 ms, the slowest.  Hence DELAYS_MS =
60, 240, 960 ms: 11 x the slowest, then x 4 each.  torch.cuda._sleep: 2.41e6 cycles per ms; a 100 ms delay took 100.02 ms.
The two re-basing recipes (stream_cases.SYNCHRONISES) returned after the whole delay, as documented, and so did
conv_properties_composed (961 ms behind 960 ms): its second family-mode call in a row waits in the HIP runtime's hipFreeAsync
(the measurement is with its entry in stream_cases.SYNCHRONISES); theta_e_difference did too until numpy_api._where stopped
uploading its scalar."""
import threading
import time

import numpy as np
import pytest

from tests import stream_cases as S
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa

pytestmark = pytest.mark.gpu
DELAYS_MS = (60.0, 240.0, 960.0)          # >= 10 x the slowest enqueue measured (see above), x 4, x 4; none over one second
assert all(b == 4 * a for a, b in zip(DELAYS_MS, DELAYS_MS[1:])) and max(DELAYS_MS) <= 1000.0
DTYPE_ID = {np.float64: 'f64', np.float32: 'f32'}
CASES = [pytest.param(n, d, id='%s-%s' % (n, DTYPE_ID[d])) for n, r in S.RECIPES.items() for d in r.dtypes]
HOST_CASES = [pytest.param(n, d, id='%s-%s' % (n, DTYPE_ID[d])) for n in S.HOST_SUBSET for d in S.RECIPES[n].dtypes]
JOIN_TIMEOUT = 120.0                       # [s] for all threads of a test together: a hang fails the test, it does not wait

REACHED = {}                               # recipe -> the entry points its side-stream run went through (_Call.run)
_recording = []                            # the recipe being recorded, if any


def load_tables():
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from oracle import tables as tb
    from xarray_parcel_amd import adiabat_tables
    tab = tb.get_tables()
    adiabat_tables.set_tables(tab.index, tab.adiabats)


@pytest.fixture(scope='module', autouse=True)
def _library():
    """The GPU, the lookup tables of moist='table' (set before anything is in flight: replacing tables drains the device) and
    the recorder around _Call.run."""
    load_tables()
    inner = xa._Call.run

    def run(self, name, *args):
        if _recording:
            REACHED.setdefault(_recording[0], set()).add(name)
        return inner(self, name, *args)
    mp = pytest.MonkeyPatch()
    mp.setattr(xa._Call, 'run', run)
    yield
    mp.undo()


def calibrated_delay():
    """delay(ms): enqueue a kernel that keeps torch's current stream busy for about that long."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles, ms = 1_000_000, 0.0
    torch.cuda._sleep(cycles)
    torch.cuda.synchronize()
    while True:                            # a sleep long enough to time: at least 5 ms
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 5.0 or cycles >= 10 ** 11:
            break
        cycles *= 10
    assert ms >= 5.0, 'torch.cuda._sleep(%d) took %.3f ms' % (cycles, ms)
    per_ms = cycles / ms
    print('torch.cuda._sleep: %.0f cycles per ms' % per_ms)
    return lambda want_ms: torch.cuda._sleep(int(want_ms * per_ms))


@pytest.fixture(scope='session')
def delay():
    return calibrated_delay()


def _np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


class Upload:
    """to_device of the reference runs: uploads (blocking) and remembers the device tensors in the order they were asked for."""

    def __init__(self, device):
        self.device, self.dev = device, []

    def __call__(self, a):
        import torch
        self.dev.append(torch.from_numpy(a).to(self.device))
        return self.dev[-1]


class Replay:
    """to_device that hands out prepared tensors in the recorded order: nothing is uploaded while the recipe runs."""

    def __init__(self, tensors):
        self.tensors, self.i = tensors, 0

    def __call__(self, a):
        t = self.tensors[self.i]
        self.i += 1
        assert tuple(t.shape) == a.shape and str(t.dtype).endswith(str(a.dtype)), (t.shape, t.dtype, a.shape, a.dtype)
        return t


_refs = {}


def reference(name, dtype, seed=S.SEED):
    """The recipe on synchronised device inputs on the default stream, computed once and kept alive -- its blocks are never the
    later runs' outputs: (the outputs as NumPy arrays, the Upload with the device inputs)."""
    import torch
    key = (name, dtype, seed)
    if key not in _refs:
        r = S.RECIPES[name]
        up = Upload(torch.device('cuda', 0))
        torch.cuda.synchronize()
        outs = r.fn(S.grid_of(r, seed), dtype, up)
        torch.cuda.synchronize()
        _refs[key] = ([_np(o).copy() for o in outs], up, outs)
    return _refs[key][:2]


def same(got, ref, label):
    """Bit for bit: as many arrays, each of the reference's dtype and shape with equal elements (NaN equal to NaN)."""
    assert len(got) == len(ref), (label, len(got), len(ref))
    for i, (a, b) in enumerate(zip(got, ref)):
        a = _np(a)
        assert a.dtype == b.dtype and a.shape == b.shape, (label, i, a.dtype, b.dtype, a.shape, b.shape)
        if not np.array_equal(a, b, equal_nan=True):
            both_nan = (a != a) & (b != b) if a.dtype.kind == 'f' else np.zeros(a.shape, bool)
            raise AssertionError('%s: output %d differs from the reference in %d of %d elements' % (label, i, int(((a != b) & ~both_nan).sum()), a.size))


def blank(t):
    """NaN for floating inputs, zero for integers and masks."""
    if t.is_floating_point():
        t.fill_(float('nan'))
    else:
        t.zero_()


# ---- (a) side-stream ordering, device tensors ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name, dtype', CASES)
def test_side_stream(name, dtype, delay):
    import torch
    r = S.RECIPES[name]
    g = S.grid_of(r)
    ref, up = reference(name, dtype)
    bufs = [torch.empty_like(t) for t in up.dev]
    s = torch.cuda.Stream()
    blocks = name in S.SYNCHRONISES
    pending = False
    for ms in DELAYS_MS:
        for b in bufs:
            blank(b)
        torch.cuda.synchronize()
        e = torch.cuda.Event()
        _recording.append(name)
        try:
            with torch.cuda.stream(s):
                delay(ms)
                e.record()
                for b, t in zip(bufs, up.dev):
                    b.copy_(t, non_blocking=True)
                t0 = time.perf_counter()
                outs = r.fn(g, dtype, Replay(bufs))
                dt = time.perf_counter() - t0
                pending = not e.query()               # before any wait
                clones = [o.clone() if hasattr(o, 'clone') else np.array(o) for o in outs]
        finally:
            _recording.clear()
        s.synchronize()
        print('%-36s %s enqueue %8.3f ms behind a delay of %g ms, event pending: %s' % (name, DTYPE_ID[dtype], 1e3 * dt, ms, pending))
        if pending or blocks:
            break
    if blocks:
        assert not pending, '%s is listed as synchronising (%s) and returned with the delay still running' % (name, S.SYNCHRONISES[name])
    else:
        assert pending, ('delay too short: %s returned after %.3f ms with the event behind a %g ms delay complete -- the call '
                         'blocks, or its enqueue takes longer than every delay of the ladder' % (name, 1e3 * dt, ms))
    same(outs, ref, name + ' outputs')
    same(clones, ref, name + ' clones')


# ---- (b) host buffers on a side stream ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, dtype', HOST_CASES)
def test_host_buffers_on_a_side_stream(name, dtype, delay, monkeypatch):
    import torch
    r = S.RECIPES[name]
    ref, _ = reference(name, dtype)
    s = torch.cuda.Stream()
    handed = []

    def run(self, entry, *args):                      # _Call.run, with the side stream where it passes NULL
        lib = L.init(None if self.device is None else self.device.index)
        stream = s.cuda_stream if self.device is None else torch.cuda.current_stream(self.device).cuda_stream
        handed.append(self.device is None)
        args = [xa._ptr(a) if isinstance(a, np.ndarray) or xa._is_torch(a) else a for a in args]
        L.check(getattr(lib, entry)(*args, stream))
    monkeypatch.setattr(xa._Call, 'run', run)
    held = []                                         # every host buffer stays alive until the stream has drained, come what may

    def keep(a):
        held.append(a)
        return a
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay(DELAYS_MS[0])
    try:
        outs = r.fn(S.grid_of(r), dtype, keep)
        held.append(outs)
        same(outs, ref, name + ' host buffers')        # no synchronisation by the test: the call's own
        assert handed and all(handed), 'the recipe made device calls out of host arrays'
    finally:
        s.synchronize()


# ---- (c) concurrent callers -----------------------------------------------------------------------------------------------------
def run_threads(plans, rounds):
    """One host thread and one fresh stream per plan [(recipe, dtype, seed), ...]: all start together and run their plan
    `rounds` times without synchronising between recipes; every result must equal that thread's serial reference."""
    import torch
    ups = [[reference(*job)[1] for job in plan] for plan in plans]            # serial references first, on the default stream
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in plans]
    barrier = threading.Barrier(len(plans))
    results, errors = [[] for _ in plans], []

    def work(i):
        try:
            with torch.cuda.stream(streams[i]):
                barrier.wait(timeout=JOIN_TIMEOUT)
                for _ in range(rounds):
                    for (name, dtype, seed), up in zip(plans[i], ups[i]):
                        r = S.RECIPES[name]
                        results[i].append(((name, dtype, seed), r.fn(S.grid_of(r, seed), dtype, Replay(up.dev))))
            streams[i].synchronize()
        except BaseException as exc:                                           # re-raised in the main thread
            errors.append((i, exc))
    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(plans))]
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN_TIMEOUT
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [i for i, t in enumerate(threads) if t.is_alive()]
    if alive:
        pytest.fail('threads %s still running after %g s' % (alive, JOIN_TIMEOUT))
    if errors:
        raise errors[0][1]
    for i, plan in enumerate(plans):
        assert len(results[i]) == rounds * len(plan)
        for job, outs in results[i]:
            same(outs, reference(*job)[0], 'thread %d %s' % (i, job[0]))


def test_four_threads_four_streams():
    """Each thread its own stream, its own seed and (alternating) dtype; five rounds of the multi-kernel recipes -- family, table,
    fused, densify, bundle, chains -- and a handful of single-kernel ones."""
    plans = [[(name, (np.float64, np.float32)[i % 2], S.SEED + 1 + i) for name in S.THREAD_RECIPES] for i in range(4)]
    for i in (1, 3):
        plans[i].reverse()                                                     # not in lock step
    run_threads(plans, rounds=5)


def test_persistent_kernels_on_two_streams():
    run_threads([[(S.PERSISTENT[0], np.float32, S.SEED)], [(S.PERSISTENT[1], np.float32, S.SEED)]], rounds=1)


# ---- (d) xp_last_error is thread-local ------------------------------------------------------------------------------------------
def test_last_error_is_thread_local():
    """Two threads make different argument errors in xp_hydrostatic_height (they return before any launch), meet, and read:
    each its own message."""
    import ctypes as C
    from tests import hydrostatic_cases as HK
    lib = L.init(0)
    p, t, td, q, base = (np.ascontiguousarray(a) for a in HK.inputs(12, 8, seed=2))
    views = [L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 12, 8, 8, 1) for a in (p, t, td)]
    z, th = np.zeros((12, 8)), np.zeros(8)
    bad = ((5, L.HUM_DEWPOINT, 'nlayer'), (1, 2, 'humidity'))                   # (nlayer, humidity kind, the word in the message)
    barrier = threading.Barrier(2)
    got, errors = [None, None], []

    def work(i):
        try:
            nlayer, hum, _ = bad[i]
            o = L.HydrostaticOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, height=z.ctypes.data)
            o.thickness[0] = th.ctypes.data
            layers = (L.WindLayer * 1)(L.WindLayer(L.LAYER_PRESSURE, 0, 900.0, 500.0))
            for _ in range(20):
                rc = lib.xp_hydrostatic_height(views[0], views[1], views[2], base.ctypes.data, nlayer, layers,
                                               L.HydrostaticOpts(hum, 0), o, None)
                barrier.wait(timeout=JOIN_TIMEOUT)                               # both calls made ...
                msg = lib.xp_last_error().decode()
                barrier.wait(timeout=JOIN_TIMEOUT)                               # ... both messages read
                got[i] = (rc, msg)
                assert rc == L.XP_E_ARG and bad[i][2] in msg and bad[1 - i][2] not in msg, (i, rc, msg)
        except BaseException as exc:
            barrier.abort()
            errors.append(exc)
    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for th_ in threads:
        th_.start()
    for th_ in threads:
        th_.join(JOIN_TIMEOUT)
    assert not any(th_.is_alive() for th_ in threads)
    real = [e for e in errors if not isinstance(e, threading.BrokenBarrierError)] or errors
    if real:
        raise real[0]
    assert got[0][1] != got[1][1]


# ---- (e) another current device -------------------------------------------------------------------------------------------------
def test_another_current_device():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs: torch.cuda.device_count() = %d' % torch.cuda.device_count())
    refs = {name: reference(name, np.float64) for name in S.OTHER_DEVICE_RECIPES}    # inputs and references on cuda:0
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(1)
    with torch.cuda.device(1):
        for name, (ref, up) in refs.items():
            r = S.RECIPES[name]
            outs = r.fn(S.grid_of(r), np.float64, Replay(up.dev))
            assert torch.cuda.current_device() == 1, name
            assert all(o.device.index == 0 for o in outs if hasattr(o, 'device')), name
            torch.cuda.synchronize(0)
            same(outs, ref, name + ' with device 1 current')
        assert torch.cuda.memory_allocated(1) == before
    assert torch.cuda.current_device() == 0


# ---- (f) coverage closes the loop -----------------------------------------------------------------------------------------------
def test_side_stream_reached_every_entry_point():
    """What the recipes went through _Call.run in test_side_stream (a recipe that test did not run in this session is run here,
    on the default stream): every recipe reached exactly the entry points it declares, and together they reached every entry
    point of the header that takes a stream."""
    import torch
    for name, r in S.RECIPES.items():
        if name not in REACHED:
            up = reference(name, r.dtypes[0])[1]
            _recording.append(name)
            try:
                r.fn(S.grid_of(r), r.dtypes[0], Replay(up.dev))
            finally:
                _recording.clear()
            torch.cuda.synchronize()
    for name, r in S.RECIPES.items():
        assert REACHED[name] == set(r.entries), (name, sorted(REACHED[name] ^ set(r.entries)))
    declared = S.header_stream_entries() - set(S.EXEMPT)
    reached = set().union(*REACHED.values())
    assert reached == declared, sorted(reached ^ declared)
