"""Perturbations of a model walk: what its result must NOT depend on.

A walk strings a few thousand launches together over five streams (the calling stream, three trunk streams, the
weight-gradient companion) and allocates its intermediates with torch.empty.  Two things can be wrong there without any
kernel being wrong, and neither shows in a fresh process or in a loop of identical steps:

  stale memory   a buffer that is read before it is written sees zeros in a fresh process and last step's (identical)
                 values in a loop.  fill_free_memory() makes every block a later torch.empty can return hold one byte
                 value: 0xFF is NaN in f32 / bf16 / f16, 255 in the u8 pool indices and -1 as an int; 0x00 is the
                 fresh-process condition.
  stream timing  a consumer that lacks a wait usually still runs after its producer, because the host enqueues slower than
                 the device drains.  delayed() makes one stream late by a known time (ds6g_debug_occupy_cus, the rehearsal
                 kernel: one workgroup asleep for `micros`, it always drains): a late producer makes a consumer without a
                 wait read the fill byte, a late reader makes an early reuse overwrite what it still needs.

Recorder wraps the library's entry points and checks the launch discipline that _fork()'s docstring states.

No fixtures here: the tests import this module (as tests/moat.py).  Every wrapper is put on the instance and taken off in a
finally; nothing process-wide is changed.
"""
import contextlib
import gc
import re
import time

import torch

MIB = 1 << 20
SMALL_MAX = MIB                       # torch's caching allocator: requests up to 1 MiB are served from the small pool
CHECK_SIZES = (4, 4 << 10, MIB, 8 * MIB, 64 * MIB)
MAX_MICROS = 2_000_000                # ds6g_debug_occupy_cus refuses more
STREAM_NAMES = ("trunk0", "trunk1", "trunk2", "wgrad", "main")


def model_streams(model):
    """the streams a walk of `model` launches and allocates on, as they exist now (the side streams are created lazily by
    the first step): the calling stream, model._side_streams, every stream of model._wg_map"""
    out = [torch.cuda.current_stream(model.device)]
    out += list(model._side_streams or [])
    out += list(model._wg_map.values())
    return out


@contextlib.contextmanager
def no_gc():
    """from a fill to the end of the step it is for, the cyclic garbage collector does not run: a dropped model is cyclic
    garbage, and collecting it after the fill hands the allocator blocks that hold the model's old values, not the fill
    byte (and collecting it inside a 12 ms step doubles the step's wall time).  Collects once on entry."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _fill(t, byte):
    if t.numel() % 8 == 0:
        word = int.from_bytes(bytes([byte]) * 8, "little", signed=True)
        t.view(torch.int64).fill_(word)
    else:
        t.fill_(byte)


def _free_blocks(raw, device_index):
    """(stream, pool kind, size) of every free block of the allocator's default pool that a torch.empty on one of the raw
    stream handles could get (a captured graph's private pool serves only its capture)"""
    out = []
    for seg in torch.cuda.memory_snapshot():
        if seg["device"] != device_index or seg["stream"] not in raw:
            continue
        if tuple(seg.get("segment_pool_id", (0, 0))) != (0, 0):
            continue
        for b in seg["blocks"]:
            if b["state"] == "inactive":
                out.append((seg["stream"], seg["segment_type"], int(b["size"])))
    return out


def fill_free_memory(byte, streams, large_bytes=128 * MIB, small_bytes=8 * MIB):
    """Every block a later torch.empty on one of `streams` can return holds `byte` -> torch.cuda.memory_reserved().

    The caching allocator keeps its free blocks per stream, in a small pool (requests <= 1 MiB) and a large one.  Under each
    stream this allocates one block of large_bytes and small_bytes in 1 MiB tensors (room for the step that follows: the
    caller checks that memory_reserved() did not grow, i.e. that the step took nothing the fill had not seen), then takes
    every remaining free block of the stream by asking for exactly its size - the allocator's best fit hands out that very
    block - until the allocator's own snapshot shows no free block left.  All of it is filled on its stream and dropped."""
    assert 0 <= byte <= 0xFF and large_bytes >= max(CHECK_SIZES) + 8 * MIB and small_bytes >= 2 * MIB
    dev = torch.cuda.current_device()
    by_raw = {s.cuda_stream: s for s in streams}
    held = []

    def take(stream, nbytes):
        with torch.cuda.stream(stream):
            t = torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")
            _fill(t, byte)
        held.append(t)

    for s in by_raw.values():
        take(s, large_bytes)
        for _ in range(small_bytes // MIB):
            take(s, MIB)
    for _ in range(8):
        free = _free_blocks(set(by_raw), dev)
        if not free:
            break
        # largest first: an exact-size request can only be served by a block of exactly that size while larger ones exist
        for raw, kind, size in sorted(free, key=lambda f: -f[2]):
            # a free small-pool block can be a whole 2 MiB segment, which no single small-pool request covers
            take(by_raw[raw], min(size, SMALL_MAX) if kind == "small" else size)
    else:
        raise AssertionError(f"fill_free_memory: free blocks remain after 8 sweeps: {_free_blocks(set(by_raw), dev)[:8]}")
    torch.cuda.synchronize()
    del held
    return torch.cuda.memory_reserved()


def assert_filled(byte, streams):
    """fresh torch.empty tensors of 4 B, 4 KiB, 1 MiB, 8 MiB and 64 MiB on each stream hold nothing but `byte`, and
    allocating them took no new segment: without this a fill that missed a pool would let every test pass"""
    reserved = torch.cuda.memory_reserved()
    for s in streams:
        for n in CHECK_SIZES:
            with torch.cuda.stream(s):
                t = torch.empty(n, dtype=torch.uint8, device="cuda")
                host = t.cpu()   # compared on the host: a comparison on the device would put its own result into the pool
            ok = bool((host == byte).all())
            assert ok, f"a fresh {n}-byte tensor on stream {s.cuda_stream:#x} holds bytes other than {byte:#04x}"
            del t
    assert torch.cuda.memory_reserved() == reserved, "the fill left no room: a fresh tensor took a new segment"


def fill_workspaces(model, byte):
    """the persistent per-stream scratch (model._ws_main, every model._ws_side) holds `byte`: no kernel may rely on what
    an earlier launch left there"""
    torch.cuda.synchronize()
    for ws in [model._ws_main] + list(model._ws_side.values()):
        _fill(ws.buf, byte)
    torch.cuda.synchronize()


def _companion_bound(model):
    """would model._wg_launch send a launch made now to a companion stream, and to which (None: not yet created)?"""
    from deepsense6g_tii_amd import ops
    if not (model.multi_stream and model.overlap_wgrad):
        return False, None
    raw = ops._stream()
    if not model.overlap_wgrad_trunks and raw in model._ws_side:
        return False, None
    return True, model._wg_map.get(raw)


class _Wrapped:
    """instance-level wrappers of _fork / _join / _wg_launch / _wg_join, removed on exit (the class's methods show again)"""
    NAMES = ("_fork", "_join", "_wg_launch", "_wg_join")

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        m = self.model
        assert not any(n in m.__dict__ for n in self.NAMES), "the walk's stream methods are wrapped already"
        orig = {n: getattr(m, n) for n in self.NAMES}
        for n in self.NAMES:
            object.__setattr__(m, n, self._wrap(n, orig[n]))
        return self

    def __exit__(self, *exc):
        for n in self.NAMES:
            self.model.__dict__.pop(n, None)
        return False

    def _wrap(self, name, fn):
        before, after = getattr(self, "before" + name, None), getattr(self, "after" + name, None)

        def call(*a, **k):
            if before is not None:
                before(*a, **k)
            out = fn(*a, **k)
            if after is not None:
                after(*a, **k)
            return out
        return call


class delayed(_Wrapped):
    """`with delayed(model, which, micros) as d:` - the stream named by `which` runs late by `micros` at every point where
    another stream has to wait for it.  "trunk0" / "trunk1" / "trunk2": a sleeper goes onto that trunk stream after each
    fork's wait (the trunk's kernels, and the join that waits for them, come `micros` later).  "wgrad": onto the companion
    stream before each weight-gradient launch that goes there.  "main": onto the calling stream after each join (_join and
    _wg_join), so what the calling stream produces next - and the next fork or companion launch must wait for - is late.
    d.injections counts the sleepers."""

    def __init__(self, model, which, micros):
        super().__init__(model)
        assert which in STREAM_NAMES and 0 < micros <= MAX_MICROS, (which, micros)
        self.which, self.micros, self.injections = which, int(micros), 0

    def _sleep(self, raw):
        from deepsense6g_tii_amd._lib import lib
        lib().debug_occupy_cus(1, 0, self.micros, raw)
        self.injections += 1

    def after_fork(self):
        if self.which.startswith("trunk"):
            self._sleep(self.model._side_streams[int(self.which[-1])].cuda_stream)

    def before_wg_launch(self, fn, keep):
        if self.which == "wgrad":
            goes, side = _companion_bound(self.model)
            if goes and side is not None:
                self._sleep(side.cuda_stream)

    def _main(self):
        from deepsense6g_tii_amd import ops
        if self.which == "main":
            self._sleep(ops._stream())

    def after_join(self):
        self._main()

    def after_wg_join(self):
        self._main()


class timed(_Wrapped):
    """`with timed(model) as t:` - t.longest is the longest host time [s] between a _fork() and its _join(), t.sections
    their number: a consumer that does not wait is enqueued within that time of its producer's stream being forked"""

    def __init__(self, model):
        super().__init__(model)
        self.longest, self.sections, self._t0 = 0.0, 0, None

    def after_fork(self):
        self._t0 = time.perf_counter()

    def before_join(self):
        assert self._t0 is not None, "_join() without a _fork()"
        self.longest = max(self.longest, time.perf_counter() - self._t0)
        self.sections += 1
        self._t0 = None


def stream_entry_points():
    """names (without ds6g_) of the C entry points whose last argument is the stream, from include/ds6g.h"""
    from deepsense6g_tii_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return [m.group(1) for m in re.finditer(r"\bint\s+ds6g_(\w+)\s*\(([^)]*?)\bvoid\s*\*\s*stream\s*\)\s*;", text)]


class Recorder(_Wrapped):
    """`with Recorder(model) as r:` - every library launch is recorded with its stream and checked against the discipline
    of TransFuser._fork: between _fork() and _join() nothing is launched on the calling stream, every launch is on the
    calling stream, a trunk stream or a companion stream, and r.outstanding (companion streams launched on since the last
    _wg_join()) is empty when the walk is over.  r.launches: [(entry point, raw stream, inside a fork section)]."""

    def __init__(self, model):
        super().__init__(model)
        self.launches, self.violations, self.outstanding = [], [], set()
        self.forked, self.calling, self.sections, self.joins = False, None, 0, 0

    def __enter__(self):
        from deepsense6g_tii_amd._lib import lib
        from deepsense6g_tii_amd import ops
        super().__enter__()
        self.calling = ops._stream()
        self._lib, self._orig = lib(), {}
        for name in stream_entry_points():
            self._orig[name] = getattr(self._lib, name)
            setattr(self._lib, name, self._entry(name, self._orig[name]))
        return self

    def __exit__(self, *exc):
        for name, fn in self._orig.items():
            setattr(self._lib, name, fn)
        return super().__exit__(*exc)

    def _entry(self, name, fn):
        def call(*args):
            raw = int(args[-1] or 0)
            m = self.model
            self.launches.append((name, raw, self.forked))
            trunks = {s.cuda_stream for s in (m._side_streams or [])}
            comps = {s.cuda_stream for s in m._wg_map.values()}
            if self.forked and raw == self.calling:
                self.violations.append(f"{name} on the calling stream between _fork() and _join()")
            if raw != self.calling and raw not in trunks and raw not in comps:
                self.violations.append(f"{name} on stream {raw:#x}: not the calling, a trunk or a companion stream")
            if raw in comps:
                self.outstanding.add(raw)
            return fn(*args)
        return call

    def before_fork(self):
        assert not self.forked, "_fork() inside a fork section"

    def after_fork(self):
        self.forked = True
        self.sections += 1

    def before_join(self):
        self.forked = False

    def after_wg_join(self):
        self.outstanding.clear()
        self.joins += 1
