"""The device ops with two streams of the library in flight at once, and with several host threads inside libzignal_hip.so at once.

Everything else in the suite runs one host thread and (almost always) one stream, so each call's scratch is reused on the stream that freed
it and no cross-stream wait is ever needed. Here:

A. one host thread, streams A and B: a scratch block freed by a call on A that has not run yet is taken by the same op on B. Both streams
   start behind an event of a third stream that is busy for some milliseconds, so the host has issued the whole backlog, the A call and the
   B call before the device starts any of them; then A's backlog (every call of it in A's block) and B's call run side by side unless B
   waits for the block's event. Asserted: A's event is still pending when B's call returns, B's call took no fresh device memory, and A's
   result, B's result and every backlog result equal the oracle. Also a smaller request into a larger block, one block going round three
   streams twice, and all of it again in child processes whose cache is capped (ZIGNAL_HIP_SCRATCH_CACHE_MB=16 and =0: results only, the
   block is then freed rather than handed over).
B. eight host threads, each on its own stream, each running its own shuffle of about forty (op, input, expected) cases three times: the
   scratch cache, the Lanczos axis-table LRU (more than 64 geometries), first-use tables (in a fresh child process), caller-made tables,
   the codecs, the host-pointer layer's band streams, and the per-thread error text.
C. a zg_graph_* capture (thread-local capture mode) and its replays on one thread while three others run eager work, and a graph captured
   on a thread that has exited.

Every expected value comes from the CPU oracle (tests/fast_ref.py for FAST), computed serially before any concurrent work starts; every
comparison is bit for bit."""
import concurrent.futures as cf
import ctypes as C
import os
import random
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import zignal_amd as zg  # noqa: E402
from zignal_amd import _lib as L  # noqa: E402
from tests.util import assert_bits_equal  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
KP = zg.KEYPOINT_DTYPE.itemsize
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    assert_bits_equal(np.ascontiguousarray(got), np.ascontiguousarray(want), what)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _err(lib):
    return (lib.zg_last_error() or b"").decode()


# ---- the ops ---------------------------------------------------------------------------------------------------------------------------
class Op:
    """make(seed) -> host inputs; alloc(ins) -> device outputs; call(ins, outs) enqueues on the current stream and allocates nothing;
    want(host inputs) -> expected arrays; fetch(ins, outs) -> the arrays compared with them (the inputs for an in-place op)."""

    def __init__(self, name, make, call, want, alloc=None, inplace=False, post=None):
        self.name, self.make, self.call, self.want, self.inplace, self.post = name, make, call, want, inplace, post
        self.alloc = alloc or (lambda ins: [] if inplace else [torch.empty_like(ins[0])])

    def fetch(self, ins, outs):
        got = [t.cpu().numpy() for t in (ins if self.inplace else outs)]
        return self.post(got) if self.post else got


def _simple(name, make, method, oracle_fn, inplace=False):
    if inplace:
        return Op(name, make, lambda ins, outs: method(zg.Image(ins[0]), zg.Image(ins[0])), lambda h: [oracle_fn(h[0])], inplace=True)
    return Op(name, make, lambda ins, outs: method(zg.Image(ins[0]), zg.Image(outs[0])), lambda h: [oracle_fn(h[0])])


def _skew(o, seed, shape):
    """Frames whose histograms differ in shape (a narrow dark band, a bright block, the full range)."""
    a = o.synth_u8(seed, shape)
    k = seed % 3
    return a if k == 0 else (a // 4 + 30).astype(np.uint8) if k == 1 else (a // 2 + 100).astype(np.uint8)


def _fast_op(o, shape, cap):
    from tests import fast_ref as F

    def make(seed):  # noise: thousands of corners, another list for every seed
        return [o.synth_u8(400 + seed, shape)]

    def alloc(ins):
        return [torch.zeros(cap * KP, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")]

    def want(h):
        w = F.detect_fast(h[0], 20, 9, True)
        assert 0 < len(w) <= cap
        return [np.array([len(w)], np.int32), w.view(np.uint8).reshape(-1)]

    def post(got):
        n = int(got[1][0])
        return [got[1], got[0][:min(n, cap) * KP]]
    return Op("fast_detect_into", make, lambda ins, outs: zg.Fast(20, True, 9).detect_into(zg.Image(ins[0]), outs[0], outs[1], cap), want, alloc, post=post)


def _pipeline_op(o, shape, n):
    rows, cols = shape
    orows, ocols = rows * 3 // 4, cols * 3 // 4
    pipe = zg.Pipeline([zg.Step.resize(orows, ocols, zg.Interpolation.lanczos), zg.Step.gaussian_blur(2.0), zg.Step.edges_sobel()])

    def want(h):
        lan = o.method(o.LANCZOS)
        res = []
        for x in h[0]:
            g = o.gaussian_blur(o.resize(x, (orows, ocols), lan), 2.0)
            res.append(o.convert(o.sobel(o.convert(g, zg.CS_RGBA, zg.CS_GRAY, np.uint8, 1)), zg.CS_GRAY, zg.CS_RGBA, np.uint8, 4))
        return [np.stack(res)]
    return Op("pipeline_run", lambda seed: [np.stack([o.synth_u8(500 + 10 * seed + i, (rows, cols, 4)) for i in range(n)])],
              lambda ins, outs: pipe.run(ins[0], out=outs[0]), want,
              lambda ins: [torch.empty((n, orows, ocols, 4), dtype=torch.uint8, device="cuda")])


K7 = ((np.arange(49, dtype=np.float32).reshape(7, 7) % 5 - 1.5) / 37.0).astype(np.float32)


def section_a_ops(o, small=False):
    """The ops of section A, each with a different owner of its scratch. small: the sizes section B mixes in."""
    def sh(r, c):
        return (r // 4 + 3, c // 4 + 5) if small else (r, c)

    def u8(shape, base):
        return lambda seed: [o.synth_u8(base + seed, shape)]

    def f32(shape, base):
        return lambda seed: [o.synth_f32(base + seed, shape)]

    def canny_frames(shape):
        def make(seed):  # a thin frame of weak strokes lit from one strong end on even seeds, noise on odd ones: different images
            a = o.synth_u8(130 + seed, shape)
            if seed % 2 == 0:
                a = (a // 8 + 60).astype(np.uint8)
                a[8, 8:-8] = 110; a[8:-8, -9] = 110; a[-9, 8:-8] = 110; a[8, 8:16] = 255
            return [a]
        return make
    binary = lambda shape: (lambda seed: [np.where(o.synth_u8(170 + seed, shape) > 247 + seed % 3, 255, 0).astype(np.uint8)])  # noqa: E731
    ops = [
        _simple("gaussian_blur_2.5_rgba_u8", u8(sh(2048, 2048) + (4,), 100), lambda s, d: s.gaussian_blur(2.5, out=d), lambda a: o.gaussian_blur(a, 2.5)),
        _simple("gaussian_blur_2.0_rgba_f32", f32(sh(1024, 1024) + (4,), 110), lambda s, d: s.gaussian_blur(2.0, out=d), lambda a: o.gaussian_blur(a, 2.0)),
        _simple("gaussian_blur_2.0_f32_plane", f32(sh(1536, 2048), 120), lambda s, d: s.gaussian_blur(2.0, out=d), lambda a: o.gaussian_blur(a, 2.0)),
        _simple("box_blur_7", u8(sh(1024, 1024) + (4,), 140), lambda s, d: s.box_blur(7, out=d), lambda a: o.box_blur(a, 7)),
        _simple("sharpen_7", u8(sh(1536, 1024), 150), lambda s, d: s.sharpen(7, out=d), lambda a: o.sharpen(a, 7)),
        _simple("canny", canny_frames(sh(1024, 1024)), lambda s, d: s.canny(1.0, 30, 90, out=d), lambda a: o.canny(a, 1.0, 30, 90)),
        _simple("shen_castan", canny_frames(sh(768, 1024)), lambda s, d: s.shen_castan(out=d), lambda a: o.shen_castan(a)),
        _simple("dilate_binary_x3", binary(sh(1024, 1024)), lambda s, d: s.dilate_binary(CROSS, 3, out=d), lambda a: o.morph(a, CROSS, 3, 0)),
        _simple("median_blur_in_place", u8(sh(768, 1024), 180), lambda s, d: s.median_blur(2, out=d), lambda a: o.order_statistic_blur(a, 2, 0, 0.5, 2),
                inplace=True),
        _simple("convolve_7x7", u8(sh(512, 768) + (4,), 190), lambda s, d: s.convolve(K7, 2, out=d), lambda a: o.convolve(a, K7, 2)),
        Op("equalize", lambda seed: [_skew(o, 200 + seed, sh(1024, 1024) + (3,))], lambda ins, outs: zg.Image(ins[0]).equalize(),
           lambda h: [o.equalize(h[0].copy())], inplace=True),
        _pipeline_op(o, sh(256, 384), 2),
        _fast_op(o, sh(1024, 1024), 1 << 16),
    ]
    return {op.name: op for op in ops}


A_NAMES = ("gaussian_blur_2.5_rgba_u8", "gaussian_blur_2.0_rgba_f32", "gaussian_blur_2.0_f32_plane", "box_blur_7", "sharpen_7", "canny", "shen_castan",
           "dilate_binary_x3", "median_blur_in_place", "convolve_7x7", "equalize", "pipeline_run", "fast_detect_into")


# ---- section A -------------------------------------------------------------------------------------------------------------------------
_GATE = {}
_WANTS = {}  # (op name, seed) -> (host inputs, expected): the oracle runs once per input in this process
WANTS_DIR = "ZIGNAL_TEST_WANTS_DIR"  # set for the child processes of this module: the oracle's values as the parent computed them


def _want(op, seed):
    key = (op.name, seed)
    if key not in _WANTS:
        host = op.make(seed)
        path = os.path.join(os.environ[WANTS_DIR], f"{op.name}-{seed}.npz") if os.environ.get(WANTS_DIR) else None
        if path and os.path.exists(path):
            with np.load(path) as z:
                want = [z[f"arr_{i}"] for i in range(len(z.files))]
        else:
            want = op.want([x.copy() for x in host])
            if path:
                np.savez(path, *want)
        _WANTS[key] = (host, want)
    return _WANTS[key]


def _hold(streams, rounds=16):
    """The streams wait for an event of a third stream that is busy for some milliseconds (passes over a 1 GiB buffer): what the host
    enqueues on them meanwhile starts together, later. Device work, not a host sleep: the host runs on at once."""
    if not _GATE:
        _GATE["buf"] = torch.zeros(1 << 30, dtype=torch.uint8, device="cuda")
        _GATE["stream"] = torch.cuda.Stream()
        torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(_GATE["stream"]):
        for _ in range(rounds):
            _GATE["buf"].add_(1)
        ev.record()
    for s in streams:
        s.wait_event(ev)
    return ev


def _free():
    return torch.cuda.mem_get_info()[0]


def handover(op, b_op=None, backlog=6, check_window=True, report=print):
    """Section A, steps 1-5, for one op. b_op: the op of the B call when it differs in size (smaller into larger)."""
    lib = zg.lib()
    b_op = b_op or op
    pairs = {"A": _want(op, 1), "B": _want(b_op, 2), "W": _want(op, 3)}
    host, want = {k: v[0] for k, v in pairs.items()}, {k: v[1] for k, v in pairs.items()}
    assert any(not np.array_equal(a, b) for a, b in zip(want["A"], want["W"])), f"{op.name}: A and the backlog give the same result"
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ins = {"A": [_cuda(x) for x in host["A"]], "B": [_cuda(x) for x in host["B"]], "warm": [_cuda(x) for x in host["W"]]}
    outs = {"A": op.alloc(ins["A"]), "B": b_op.alloc(ins["B"]), "warm": op.alloc(ins["warm"])}
    log_ins = [[_cuda(x) for x in host["W"]] for _ in range(backlog)]
    log_outs = [op.alloc(i) for i in log_ins]
    torch.cuda.synchronize()
    lib.zg_trim_scratch()
    before = _free()
    for s in (sa, sb):  # first-use tables, code objects, the streams themselves; the op's blocks enter the cache once
        with torch.cuda.stream(s):
            op.call(ins["warm"], outs["warm"])
        s.synchronize()
    footprint = before - _free()
    held = _hold((sa, sb))
    with torch.cuda.stream(sa):
        for i, t in zip(log_ins, log_outs):
            op.call(i, t)
        op.call(ins["A"], outs["A"])
        ev = torch.cuda.Event()
        ev.record()
    free0 = _free()
    with torch.cuda.stream(sb):
        b_op.call(ins["B"], outs["B"])
    busy = not ev.query()
    took = free0 - _free()
    still_held = not held.query()
    sa.synchronize()
    sb.synchronize()
    report(f"section A {op.name}: scratch footprint {footprint / MIB:.1f} MiB, A busy at B's return: {busy} (streams still held: {still_held}), "
           f"device memory B's call took: {took / MIB:.2f} MiB")
    if check_window:
        assert busy, f"{op.name}: the event on A had completed when B's call returned: the hazard window was not open"
        assert took < MIB, f"{op.name}: B's call took {took} bytes of fresh device memory: it did not take A's block (no block is below 1 MiB)"
    for k, (o_, i_, t_) in {"A": (op, ins["A"], outs["A"]), "B": (b_op, ins["B"], outs["B"])}.items():
        for n, (g, w) in enumerate(zip(o_.fetch(i_, t_), want[k])):
            _same(g, w, f"{op.name}: stream {k}, output {n}")
    for j, (i_, t_) in enumerate(zip(log_ins, log_outs)):
        for n, (g, w) in enumerate(zip(op.fetch(i_, t_), want["W"])):
            _same(g, w, f"{op.name}: backlog call {j} on A, output {n}")


def rotation(op, check_window=True, report=print):
    """One block round three streams twice: A -> B -> C -> A -> B -> C, every call on its own input, each taking the block the call before
    it has just freed on another stream."""
    lib = zg.lib()
    host, want = zip(*[_want(op, 10 + i) for i in range(6)])
    streams = [torch.cuda.Stream() for _ in range(3)]
    ins = [[_cuda(x) for x in h] for h in host]
    outs = [op.alloc(i) for i in ins]
    warm_in, warm_out = [_cuda(x) for x in host[0]], op.alloc(ins[0])
    torch.cuda.synchronize()
    lib.zg_trim_scratch()
    for s in streams:
        with torch.cuda.stream(s):
            op.call(warm_in, warm_out)
        s.synchronize()
    _hold(streams)
    prev, window = None, []
    for k in range(6):
        free0 = _free()
        with torch.cuda.stream(streams[k % 3]):
            op.call(ins[k], outs[k])
            ev = torch.cuda.Event()
            ev.record()
        if prev is not None:
            window.append((not prev.query(), free0 - _free()))
        prev = ev
    for s in streams:
        s.synchronize()
    report(f"section A rotation {op.name}: (previous call busy, device memory taken) per hand-over: {window}")
    if check_window:
        assert all(b for b, _ in window), f"a call had completed before the next stream's call returned: {window}"
        assert all(t < MIB for _, t in window), f"a call took fresh device memory instead of the block going round: {window}"
    for k in range(6):
        for n, (g, w) in enumerate(zip(op.fetch(ins[k], outs[k]), want[k])):
            _same(g, w, f"rotation {op.name}: call {k} on stream {'ABC'[k % 3]}, output {n}")


def _smaller_blur(o):
    """gaussian_blur(2.5) on 1408 x 2048: a temp plane of 0.69 of the 2048^2 one, inside the best-fit rule's (half, all]."""
    return _simple("gaussian_blur_2.5_rgba_u8_1408", lambda seed: [o.synth_u8(100 + seed, (1408, 2048, 4))], lambda s, d: s.gaussian_blur(2.5, out=d),
                   lambda a: o.gaussian_blur(a, 2.5))


def _rotation_op(o):
    return _simple("gaussian_blur_2.5_rgba_u8_1024x1536", lambda seed: [o.synth_u8(300 + seed, (1024, 1536, 4))], lambda s, d: s.gaussian_blur(2.5, out=d),
                   lambda a: o.gaussian_blur(a, 2.5))


def section_a_all(o, check_window):
    """Every scenario of section A in this process (the capped-cache children)."""
    ops = section_a_ops(o)
    for name in A_NAMES:
        handover(ops[name], check_window=check_window)
    handover(ops[A_NAMES[0]], b_op=_smaller_blur(o), check_window=check_window)
    rotation(_rotation_op(o), check_window=check_window)


@pytest.mark.parametrize("name", A_NAMES)
def test_a_block_freed_on_one_stream_is_handed_to_another(oracle, name):
    handover(section_a_ops(oracle)[name])


def test_a_smaller_request_takes_the_larger_block_of_another_stream(oracle):
    handover(section_a_ops(oracle)[A_NAMES[0]], b_op=_smaller_blur(oracle))


def test_a_block_goes_round_three_streams_twice(oracle):
    rotation(_rotation_op(oracle))


def _child(body, env=None, timeout=600, module="tests.test_gpu_concurrency"):
    """`body` in a fresh process, with the oracle as `o` and `module` (this one, or one that extends it) as `T`."""
    code = ("import sys; sys.path.insert(0, %r)\nfrom oracle import pyoracle as o; o.lib()\nimport %s as T\n%s\nprint('ok')\n" % (ROOT, module, body))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=dict(os.environ, **(env or {})))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def _share_wants():
    """One directory for every child process of a session: what this process has computed is written there, and whichever input has no
    file yet is computed in the child that first needs it and kept."""
    if WANTS_DIR not in os.environ:
        import tempfile
        _WANTS["dir"] = tempfile.TemporaryDirectory()
        os.environ[WANTS_DIR] = _WANTS["dir"].name
    for (name, seed), (_, want) in [kv for kv in _WANTS.items() if kv[0] != "dir"]:
        path = os.path.join(os.environ[WANTS_DIR], f"{name}-{seed}.npz")
        if not os.path.exists(path):
            np.savez(path, *want)


@pytest.mark.parametrize("cap_mb", ("16", "0"))
def test_a_capped_cache_frees_blocks_with_events_pending_and_changes_nothing(cap_mb):
    """ZIGNAL_HIP_SCRATCH_CACHE_MB is read once: a child process. Past the cap a freed block goes back to the driver while the call that used
    it is still queued, so nothing is handed over and the window conditions do not apply; every result must still equal the oracle."""
    _share_wants()
    print(_child("T.section_a_all(o, check_window=False)", {"ZIGNAL_HIP_SCRATCH_CACHE_MB": cap_mb}))


# ---- section B -------------------------------------------------------------------------------------------------------------------------
class Case:
    """run(tid) -> arrays, on the calling thread's current stream; want: the expected arrays, or one list per thread."""

    def __init__(self, name, run, want, per_thread=False):
        self.name, self.run, self.want, self.per_thread = name, run, want, per_thread

    def check(self, tid):
        got = self.run(tid)
        want = self.want[tid] if self.per_thread else self.want
        assert len(got) == len(want), self.name
        for n, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{self.name}: thread {tid}, output {n}")


def _op_case(op, seed, tag):
    host = op.make(seed)
    want = op.want([x.copy() for x in host])

    def run(tid):
        ins = [_cuda(x) for x in host]
        outs = op.alloc(ins)
        op.call(ins, outs)
        return op.fetch(ins, outs)
    return Case(f"{op.name} {tag}", run, want)


def _lanczos_lut(scale):
    x = np.arange(1025, dtype=np.float64) * 3.0 / 1024.0
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(x == 0, 1.0, 3.0 * np.sin(np.pi * x) * np.sin(np.pi * x / 3.0) / (np.pi * np.pi * x * x))
    return np.ascontiguousarray((v * scale).astype(np.float32))


def _pyramid_shapes(rows, cols, n, factor, sigma):
    from tests.test_gpu_graph_replay import _level_shape
    return [_level_shape(zg, rows, cols, factor, sigma, i) for i in range(1, n)]


def _pyramid_call(src, levels, sigmas):
    """zg_pyramid_build into levels the caller made (ImagePyramid.build allocates, which a capturing thread must not)."""
    lib = zg.lib()
    d = zg.Image(src)._desc()
    descs = (L.ZgImage * len(levels))(*[zg.Image(t)._desc() for t in levels])
    sig = (C.c_float * len(sigmas))(*sigmas)
    assert lib.zg_pyramid_build(C.byref(d), descs, sig, len(levels), _st()) == 0, _err(lib)


def section_b_cases(o, threads=8):
    from tests import fast_ref as F
    lan = o.method(o.LANCZOS)
    cases = []
    big, small = section_a_ops(o), section_a_ops(o, small=True)
    for i, name in enumerate(A_NAMES):  # the ops of section A at two sizes each, the large ones of a few only
        cases.append(_op_case(small[name], 20 + i, "small"))
    for name in ("gaussian_blur_2.0_rgba_f32", "box_blur_7", "canny", "dilate_binary_x3"):
        cases.append(_op_case(big[name], 40, "large"))
    # Lanczos resizes of Rgb(u8) and Rgba(u8): 9 cases x 8 geometries = 72 distinct ones, past the 64 entries of the axis-table LRU
    for b in range(9):
        ch = 3 + b % 2
        src = o.synth_u8(600 + b, (40, 50, ch))
        geos = [(23 + 8 * b + i, 61 + 16 * b + 2 * i) for i in range(8)]
        want = [o.resize(src, g, lan) for g in geos]

        def run(tid, src=src, geos=geos):
            d = zg.Image(_cuda(src))
            return [d.resize(g, zg.Interpolation.lanczos).to_numpy() for g in geos]
        cases.append(Case(f"lanczos resizes {b} ({ch} channels)", run, want))
    # tables the caller makes, different for every thread
    rgba = o.synth_u8(620, (60, 90, 4))
    mat = [1.0, 0.1, -0.05, 1.0, 2.0, 1.0]
    luts = [_lanczos_lut(1.0 - t / 32.0) for t in range(threads)]
    wants = []
    for lut in luts:
        om = o.method(o.LANCZOS)
        om.lanczos_lut = lut.ctypes.data
        wants.append([o.warp(rgba, (60, 90), o.AFFINE, np.array(mat, np.float32), om)])

    def run_lut(tid):
        lib = zg.lib()
        src, out = _cuda(rgba), torch.empty((60, 90, 4), dtype=torch.uint8, device="cuda")
        sd, od = zg.Image(src)._desc(), zg.Image(out)._desc()
        m = L.ZgMethod(5, 0.0, 0.0, luts[tid].ctypes.data)
        assert lib.zg_warp(C.byref(sd), C.byref(od), 1, (C.c_float * 6)(*mat), C.byref(m), _st()) == 0, _err(lib)
        return [out.cpu().numpy()]
    cases.append(Case("warp, caller's lanczos_lut", run_lut, wants, per_thread=True))
    base = np.ascontiguousarray(o.srgb_to_linear_lut(), np.float32)
    sluts = [np.ascontiguousarray(base * np.float32(1.0 - t / 64.0)) for t in range(threads)]
    wants = [[o.convert(rgba, zg.CS_RGBA, zg.CS_OKLAB, np.float32, 3, srgb_lut=s)] for s in sluts]
    cases.append(Case("convert, caller's srgb_lut", lambda tid: [zg.Image(_cuda(rgba)).convert(zg.CS_OKLAB, np.float32, srgb_lut=sluts[tid]).to_numpy()],
                      wants, per_thread=True))
    # conversions through the library's own sRGB table, and back
    photo = o.synth_u8(630, (150, 333, 4))
    for space, name in ((zg.CS_OKLAB, "oklab"), (zg.CS_LAB, "lab"), (zg.CS_XYZ, "xyz")):
        there = o.convert(photo, zg.CS_RGBA, space, np.float32, 3)
        back = o.convert(there, space, zg.CS_RGBA, np.uint8, 4)

        def run(tid, space=space, there=there):
            return [zg.Image(_cuda(photo)).convert(space, np.float32).to_numpy(),
                    zg.Image(_cuda(there)).convert(zg.CS_RGBA, np.uint8, src_space=space).to_numpy()]
        cases.append(Case(f"rgba <-> {name}", run, [there, back]))
    grey = F.photo_like(o.synth_u8(640, (400, 600)))
    cases.append(Case("ImagePyramid.build", lambda tid: [lv.to_numpy() for lv in zg.ImagePyramid.build(zg.Image(_cuda(grey)), 5, 1.3, 1.6).levels[1:]],
                      o.pyramid(grey, 5, 1.3, 1.6)[1:]))
    kp_bytes = lambda k: np.ascontiguousarray(k).view(np.uint8).reshape(-1)  # noqa: E731  (the whole keypoint list as bytes, order included)
    cases.append(Case("Fast.detect", lambda tid: [kp_bytes(zg.Fast(20, True).detect(zg.Image(_cuda(grey)), capacity=64))],
                      [kp_bytes(F.detect_fast(grey, 20, 9, True))]))
    pair = [grey, np.ascontiguousarray(grey[::2, ::2])]
    cases.append(Case("Fast.detect_batch", lambda tid: [kp_bytes(k) for k in zg.Fast(20, True).detect_batch([zg.Image(_cuda(x)) for x in pair], [20, 12])],
                      [kp_bytes(F.detect_fast(pair[0], 20, 9, True)), kp_bytes(F.detect_fast(pair[1], 12, 9, True))]))
    rng = np.random.default_rng(3)
    bimodal = np.clip(np.where(rng.random((300, 500)) < 0.4, rng.normal(190, 20, (300, 500)), rng.normal(60, 12, (300, 500))), 0, 255).astype(np.uint8)
    wi, wt = o.threshold_otsu(bimodal)

    def run_otsu(tid):
        img, t = zg.Image(_cuda(bimodal)).threshold_otsu()
        return [img.to_numpy(), np.array([t], np.int64)]
    cases.append(Case("threshold_otsu", run_otsu, [wi, np.array([wt], np.int64)]))
    k17 = ((np.arange(17 * 17, dtype=np.float32).reshape(17, 17) % 7) / 400.0).astype(np.float32)
    cases.append(Case("convolve 17x17 (taps in scratch)", lambda tid: [zg.Image(_cuda(rgba)).convolve(k17, 1).to_numpy()], [o.convolve(rgba, k17, 1)]))
    png = o.png_encode_stored(photo)
    cases.append(Case("png decode", lambda tid: [zg.Image.load_from_bytes(png, "rgba_u8").to_numpy()], [o.png_load(png, "rgba_u8")]))
    jpg = o.jpeg_encode(np.ascontiguousarray(photo[..., :3]), quality=85)
    cases.append(Case("jpeg decode", lambda tid: [zg.Image.load_from_bytes(jpg, "rgb_u8").to_numpy()], [o.jpeg_load(jpg, "rgb_u8")]))
    # the host-pointer layer, large enough for the banded route (its three streams belong to the calling thread)
    frame = o.synth_u8(650, (2048, 2048, 4))
    cases.append(Case("host gaussian_blur (banded)", lambda tid: [zg.Image(frame).gaussian_blur(1.0).to_numpy()], [o.gaussian_blur(frame, 1.0)]))
    cases.append(Case("host box_blur (banded)", lambda tid: [zg.Image(frame).box_blur(2).to_numpy()], [o.box_blur(frame, 2)]))
    return cases


def _first_use_cases(o):
    """What every thread of the fresh child calls first: an sRGB conversion, then a Lanczos resize (the first-use tables, the occupancy cache)."""
    a = o.synth_u8(660, (97, 131, 4))
    return [Case("first sRGB conversion", lambda tid: [zg.Image(_cuda(a)).convert(zg.CS_OKLAB, np.float32).to_numpy()],
                 [o.convert(a, zg.CS_RGBA, zg.CS_OKLAB, np.float32, 3)]),
            Case("first Lanczos resize", lambda tid: [zg.Image(_cuda(a)).resize((61, 83), zg.Interpolation.lanczos).to_numpy(),
                                                       zg.Image(_cuda(a[..., 0])).resize((61, 83), zg.Interpolation.lanczos).to_numpy()],
                 [o.resize(a, (61, 83), o.method(o.LANCZOS)), o.resize(np.ascontiguousarray(a[..., 0]), (61, 83), o.method(o.LANCZOS))])]


def _refusals(o):
    """Calls the library refuses on their arguments alone (nothing is launched), and what zg_last_error must then name."""
    rgba, grey = _cuda(o.synth_u8(670, (32, 48, 4))), _cuda(o.synth_u8(671, (32, 48)))
    out, wrong, gout = torch.empty_like(rgba), torch.empty((30, 48, 4), dtype=torch.uint8, device="cuda"), torch.empty_like(grey)
    keep = (rgba, out, wrong, grey, gout)
    lib = zg.lib()
    sd, od, wd, gd, god = (zg.Image(t)._desc() for t in keep)
    return keep, [
        (lambda: lib.zg_gaussian_blur(C.byref(sd), C.byref(od), C.c_float(-1.0), _st()), L.ERR_INVALID_ARGUMENT, "gaussianBlur: InvalidSigma"),
        (lambda: lib.zg_box_blur(C.byref(sd), C.byref(wd), 2, _st()), L.ERR_DIMENSION_MISMATCH, "boxBlur: 32x48 vs 30x48"),
        (lambda: lib.zg_canny(C.byref(gd), C.byref(god), C.c_float(1.0), C.c_float(90.0), C.c_float(30.0), _st()), L.ERR_INVALID_ARGUMENT,
         "canny: InvalidThreshold"),
    ]


def run_threads(o, cases, threads=8, passes=3, first=None, refuse=True):
    """Section B: `threads` workers, each on its own stream, released together; each checks `first` (in order), then its own shuffle of
    `cases` `passes` times. Worker 1 interleaves refused calls and checks the error text; worker 2 trims the scratch cache between cases;
    every other worker's error text must stay empty."""
    lib = zg.lib()
    barrier = threading.Barrier(threads)

    def worker(tid):
        stream = torch.cuda.Stream()
        done = 0
        with torch.cuda.stream(stream):
            refusals = _refusals(o) if (refuse and tid == 1) else None
            stream.synchronize()
            barrier.wait(timeout=120)
            for c in first or ():
                c.check(tid)
            expect = ""
            for p in range(passes):
                order = list(range(len(cases)))
                random.Random(1000 * tid + p).shuffle(order)
                for n, i in enumerate(order):
                    if refusals:
                        call, status, text = refusals[1][(n + p) % 3]
                        rc = call()
                        assert rc == status and text in _err(lib), f"refusal: status {rc}, error text {_err(lib)!r}, expected {status} and {text!r}"
                        expect = _err(lib)
                    cases[i].check(tid)
                    assert _err(lib) == expect, f"thread {tid}: error text {_err(lib)!r} after {cases[i].name}, expected {expect!r}"
                    if tid == 2:
                        assert lib.zg_trim_scratch() == 0
                    done += 1
        return done

    with cf.ThreadPoolExecutor(threads) as pool:
        futures = [pool.submit(worker, t) for t in range(threads)]
        failures = []
        for t, f in enumerate(futures):
            try:
                assert f.result(timeout=900) == passes * len(cases)
            except Exception as e:  # noqa: BLE001  (every worker's failure is reported, not the first only)
                failures.append(f"thread {t}: {type(e).__name__}: {e}")
    assert not failures, "\n".join(failures)


def test_b_eight_threads_each_on_its_own_stream(oracle):
    cases = section_b_cases(oracle)
    assert len(cases) >= 38
    run_threads(oracle, cases)


def test_b_first_use_tables_contended_in_a_fresh_process():
    """A fresh process has no sRGB table, no Lanczos table and no occupancy figures: eight threads ask for them at the same moment."""
    _child("T.run_threads(o, T.section_b_cases(o), first=T._first_use_cases(o))")


# ---- section C -------------------------------------------------------------------------------------------------------------------------
def _eager_threads(o, cases, n, stop, counters, release_on=None):
    """n threads, each on its own stream, checking `cases` round and round until `stop` is set (and once through at least)."""
    lib = zg.lib()

    def worker(tid):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            k = 0
            while k < len(cases) or not stop.is_set():
                cases[(k + 3 * tid) % len(cases)].check(tid)
                if tid == release_on:
                    assert lib.zg_release_graph_scratch() == 0
                k += 1
                counters[tid] = k
        return k
    pool = cf.ThreadPoolExecutor(n)
    return pool, [pool.submit(worker, t) for t in range(n)]


def test_c_capture_and_replay_beside_eager_threads(oracle):
    from tests.test_gpu_graph_replay import Capture, _sentinel
    o = oracle
    lan = o.method(o.LANCZOS)
    rows, cols = 300, 400
    frames = [(o.synth_u8(700 + s, (rows, cols, 4)), o.synth_u8(710 + s, (rows, cols))) for s in range(3)]
    shapes = _pyramid_shapes(rows, cols, 4, 1.5, 1.6)
    assert len(shapes) == 3

    def want(f):
        return [o.gaussian_blur(f[0], 2.5), o.resize(f[0], (211, 317), lan), o.canny(f[1], 1.0, 30, 90)] + o.pyramid(f[1], 4, 1.5, 1.6)[1:]
    wants = [want(f) for f in frames]
    small = section_a_ops(o, small=True)
    eager = [_op_case(small[n], 60 + i, "eager") for i, n in enumerate(A_NAMES)]
    src, gsrc = _cuda(frames[0][0]), _cuda(frames[0][1])
    outs = [torch.empty_like(src), torch.empty((211, 317, 4), dtype=torch.uint8, device="cuda"), torch.empty_like(gsrc)]
    outs += [torch.empty((r, c), dtype=torch.uint8, device="cuda") for r, c, _ in shapes]
    sigmas = [s for _, _, s in shapes]

    def calls():
        zg.Image(src).gaussian_blur(2.5, out=zg.Image(outs[0]))
        zg.Image(src).resize(zg.Image(outs[1]), zg.Interpolation.lanczos)
        zg.Image(gsrc).canny(1.0, 30, 90, out=zg.Image(outs[2]))
        _pyramid_call(gsrc, outs[3:], sigmas)

    torch.cuda.synchronize()
    stop, counters = threading.Event(), [0, 0, 0]
    pool, futures = _eager_threads(o, eager, 3, stop, counters, release_on=1)
    cap = Capture()
    try:
        deadline = time.monotonic() + 120
        while min(counters) < 1 and time.monotonic() < deadline and not any(f.done() for f in futures):
            time.sleep(0.01)  # the eager threads are under way before the capture begins
        with torch.cuda.stream(cap.stream):
            calls()  # warm-up: the Lanczos geometry's tables, the first-use tables
        cap.stream.synchronize()
        cap.record(calls)
        at_capture = list(counters)
        rounds = 0
        while rounds < 3 or (min(c - a for c, a in zip(counters, at_capture)) < 3 and time.monotonic() < deadline and not any(f.done() for f in futures)):
            k = (1, 2, 0)[rounds % 3]
            with torch.cuda.stream(cap.stream):
                src.copy_(torch.from_numpy(frames[k][0]))
                gsrc.copy_(torch.from_numpy(frames[k][1]))
                for t in outs:
                    _sentinel(t)
            cap.launch()
            for n, (t, w) in enumerate(zip(outs, wants[k])):
                _same(t.cpu().numpy(), w, f"replay {rounds} on input {'ABC'[k]} beside eager threads, output {n}")
            rounds += 1
        overlap = [c - a for c, a in zip(counters, at_capture)]
    finally:
        stop.set()
        results = []
        for t, f in enumerate(futures):
            try:
                results.append(f.result(timeout=600))
            except Exception as e:  # noqa: BLE001
                results.append(f"thread {t}: {type(e).__name__}: {e}")
        pool.shutdown()
        cap.destroy()
    assert all(isinstance(r, int) for r in results), results
    assert min(overlap) >= 3, f"eager cases finished per thread while the graph replayed: {overlap}"


def test_c_a_graph_outlives_the_thread_that_captured_it(oracle):
    """A pyramid build forks over the capturing thread's own helper streams; they are destroyed when that thread ends. The graph must not
    need them: launched from the main thread on a fresh stream, on changed inputs, and destroyed there; its memory comes back."""
    from tests.test_gpu_graph_replay import Capture, _sentinel
    o = oracle
    lib = zg.lib()
    rows, cols = 512, 768
    frames = [o.synth_u8(720 + s, (rows, cols)) for s in range(2)]
    shapes = _pyramid_shapes(rows, cols, 6, 1.5, 1.6)
    wants = [o.pyramid(f, 6, 1.5, 1.6)[1:] for f in frames]
    src = _cuda(frames[0])
    levels = [torch.empty((r, c), dtype=torch.uint8, device="cuda") for r, c, _ in shapes]
    sigmas = [s for _, _, s in shapes]
    _pyramid_call(src, levels, sigmas)  # code objects and first-use state are in the baseline
    torch.cuda.synchronize()
    lib.zg_trim_scratch()
    base = _free()
    box = {}

    def capture_and_exit():
        try:
            cap = Capture()
            with torch.cuda.stream(cap.stream):
                _pyramid_call(src, levels, sigmas)
            cap.stream.synchronize()
            cap.record(lambda: _pyramid_call(src, levels, sigmas))
            box["graph"] = cap.graph
        except BaseException as e:  # noqa: BLE001
            box["error"] = e
    t = threading.Thread(target=capture_and_exit)
    t.start()
    t.join(300)
    assert not t.is_alive() and "error" not in box, box.get("error")
    fresh = torch.cuda.Stream()
    try:
        for k in (1, 0):
            with torch.cuda.stream(fresh):
                src.copy_(torch.from_numpy(frames[k]))
                for lv in levels:
                    _sentinel(lv)
            assert lib.zg_graph_launch(box["graph"], C.c_void_p(fresh.cuda_stream)) == 0, _err(lib)
            fresh.synchronize()
            for n, (lv, w) in enumerate(zip(levels, wants[k])):
                _same(lv.cpu().numpy(), w, f"graph of an ended thread, input {'AB'[k]}, level {n + 1}")
    finally:
        assert lib.zg_graph_destroy(box["graph"]) == 0
    torch.cuda.synchronize()
    lib.zg_trim_scratch()
    assert base - _free() <= 8 * MIB, f"{base - _free()} bytes not returned after the graph was destroyed"


def test_c_an_eager_call_takes_a_block_last_used_on_a_stream_that_is_now_capturing(oracle):
    """The runtime counts a wait on an event whose stream is capturing as part of that capture, whichever thread it comes from, and
    invalidates the capture (and fails the eager call) when it comes from outside. A block the capturing stream used just before its capture
    is in the cache with such an event: another thread's eager call of the same size takes exactly that block. Both must work: the eager
    result, and the graph replayed on a changed input."""
    from tests.test_gpu_graph_replay import Capture, _sentinel
    lib = zg.lib()
    op = section_a_ops(oracle, small=True)["gaussian_blur_2.5_rgba_u8"]
    (ha, wa), (hb, wb), (hc, wc) = (_want(op, 80 + i) for i in range(3))
    src, out = _cuda(ha[0]), torch.empty(ha[0].shape, dtype=torch.uint8, device="cuda")
    other_in, other_out = _cuda(hb[0]), torch.empty(hb[0].shape, dtype=torch.uint8, device="cuda")
    cap = Capture()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op.call([other_in], [other_out])  # the other thread's stream and the code objects exist before anything is measured
    torch.cuda.synchronize()
    lib.zg_trim_scratch()
    with torch.cuda.stream(cap.stream):
        op.call([src], [out])  # the only block in the cache, its event recorded on the stream about to capture
    cap.stream.synchronize()
    box = {}

    def eager():
        try:
            with torch.cuda.stream(side):
                free0 = _free()
                op.call([other_in], [other_out])
                box["took"] = free0 - _free()
                side.synchronize()
                box["got"] = other_out.cpu().numpy()
        except BaseException as e:  # noqa: BLE001
            box["error"] = e
    g = C.c_void_p()
    with torch.cuda.stream(cap.stream):
        assert lib.zg_graph_begin_capture(cap.sp) == 0, _err(lib)
        try:
            t = threading.Thread(target=eager)
            t.start()
            t.join(120)
            op.call([src], [out])
        finally:
            rc = lib.zg_graph_end_capture(cap.sp, C.byref(g))
    assert rc == 0, _err(lib)
    cap.graph = g
    try:
        assert "error" not in box, box.get("error")
        assert box["took"] < MIB, f"the eager call took {box['took']} bytes of fresh device memory: it did not take the capturing stream's block"
        _same(box["got"], wb[0], "the eager call beside the capture")
        for host, want in ((hc, wc), (ha, wa)):
            with torch.cuda.stream(cap.stream):
                src.copy_(torch.from_numpy(host[0]))
                _sentinel(out)
            cap.launch()
            _same(out.cpu().numpy(), want[0], "replay of the capture another thread's eager call ran beside")
    finally:
        cap.destroy()
