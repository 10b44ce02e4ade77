"""Every asynchronous device entry point under graph capture, replayed on CHANGED inputs against the oracle.

Graph replay is how the library runs (bench.py captures every leg), and a replay can go wrong where no eager call can: a kernel node
that points at memory the library frees later, host-side work done at capture time that depends on pixel values, routes that only
run under capture (the pyramid's forked levels). Each row of the table: one eager warm-up, one capture on input A, then for B, C and A
the same device buffers are reloaded, every output is set to a sentinel, the graph is launched and the outputs are compared with the
oracle bit for bit. The oracle's outputs for A and B must differ, so a stale replay cannot pass. The last test (no GPU) holds the table
to include/zignal_hip.h: a new entry point cannot ship without a row here or a reason on the exemption list."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = 5

# Entry points without a row, and why. Everything else that include/zignal_hip.h exports is named by a row (ROWS) or a test below.
EXEMPT = {
    "_host": "host-pointer layer: synchronous by contract, nothing to capture",
    "zg_multi_": "several GPUs (one is available to the suite)",
    "runtime": "device, memory, stream, event and graph management: the capture machinery itself",
    "codec": "PNG / JPEG: host entropy coding; the device halves that are capturable are covered where listed",
    "host_math": "host-only arithmetic (taps, shapes, bounds): no device work",
}
RUNTIME = {"zg_init", "zg_set_device", "zg_get_device", "zg_shutdown", "zg_last_error", "zg_version", "zg_device_count", "zg_malloc", "zg_free",
           "zg_malloc_host", "zg_free_host", "zg_memcpy_h2d", "zg_memcpy_d2h", "zg_memcpy_h2d_async", "zg_memcpy_d2h_async", "zg_image_upload",
           "zg_image_download", "zg_stream_create", "zg_stream_destroy", "zg_stream_synchronize", "zg_stream_wait_event", "zg_event_create",
           "zg_event_destroy", "zg_event_record", "zg_event_synchronize", "zg_event_elapsed_ms", "zg_graph_begin_capture", "zg_graph_end_capture",
           "zg_graph_launch", "zg_graph_destroy", "zg_release_graph_scratch", "zg_trim_scratch", "zg_pixel_size", "zg_sizeof_step"}
HOST_MATH = {"zg_gaussian_kernel", "zg_lanczos_plane_weights", "zg_rotate_bounds", "zg_crop_dims", "zg_pyramid_scale", "zg_pyramid_level",
             "zg_batch_pipeline_shape"}
CODEC_PREFIXES = ("zg_png_", "zg_jpeg_")
# Entry points covered by dedicated tests below rather than by a ROWS entry.
COVERED_ELSEWHERE = {"zg_resize_lanczos_weights": "test_non_capturable_calls_refuse_and_leave_the_stream_usable",
                     "zg_threshold_otsu": "ROWS (threshold_out NULL) and the refusal test (threshold_out set)"}


def _header_entry_points():
    text = open(os.path.join(ROOT, "include", "zignal_hip.h")).read()
    return sorted(set(re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(", text)))


# ---- the table -------------------------------------------------------------------------------------------------------------------
# name -> the entry points the row drives (ctypes or through zignal_amd.Image)
ROWS = {
    "conv_separable": ["zg_conv_separable"], "conv_separable_planes": ["zg_conv_separable_planes"],
    "gaussian_blur": ["zg_gaussian_blur"], "gaussian_blur_planes": ["zg_gaussian_blur_planes"], "convolve": ["zg_convolve"],
    "box_blur": ["zg_box_blur"], "sharpen": ["zg_sharpen"], "integral": ["zg_integral"], "invert": ["zg_invert"],
    "resize": ["zg_resize"], "letterbox": ["zg_letterbox"], "warp": ["zg_warp"], "rotate_into": ["zg_rotate_into"], "extract": ["zg_extract"],
    "crop": ["zg_crop"], "flips": ["zg_flip_left_right", "zg_flip_top_bottom"], "insert": ["zg_insert"],
    "copy_fill_border": ["zg_copy", "zg_fill", "zg_set_border"], "convert": ["zg_convert"], "resize_convert": ["zg_resize_convert"],
    "devmath": ["zg_devmath_apply"], "sobel": ["zg_sobel"], "canny": ["zg_canny"], "shen_castan": ["zg_shen_castan"],
    "isef_smooth": ["zg_isef_smooth"], "order_statistic": ["zg_order_statistic_blur"], "morph": ["zg_morph"],
    "threshold_otsu": ["zg_threshold_otsu"], "threshold_adaptive": ["zg_threshold_adaptive_mean"], "autocontrast": ["zg_autocontrast"],
    "equalize": ["zg_equalize"], "motion_linear": ["zg_motion_blur_linear"], "motion_radial": ["zg_motion_blur_radial"],
    "fast": ["zg_fast_detect"], "fast_batch": ["zg_fast_detect_batch"], "pyramid_level": ["zg_pyramid_build_level"],
    "pyramid": ["zg_pyramid_build"], "batch_blur_resize": ["zg_batch_blur_resize"], "batch_pipeline": ["zg_batch_pipeline"],
}


def test_every_entry_point_has_a_replay_row_or_a_reason():
    rowed = {ep for eps in ROWS.values() for ep in eps}
    missing = []
    for ep in _header_entry_points():
        if ep in rowed or ep in COVERED_ELSEWHERE or ep in RUNTIME or ep in HOST_MATH:
            continue
        if ep.endswith("_host") or ep.startswith("zg_multi_") or ep.startswith(CODEC_PREFIXES):
            continue
        missing.append(ep)
    assert not missing, f"entry points with neither a graph-replay row nor an exemption ({'; '.join(f'{k}: {v}' for k, v in EXEMPT.items())}): {missing}"
    assert not (rowed - set(_header_entry_points())), "a row names an entry point the header does not have"


# ---- GPU side ----------------------------------------------------------------------------------------------------------------------
torch = None


def _torch():
    global torch
    if torch is None:
        torch = pytest.importorskip("torch")
    return torch


def _zg():
    _torch()
    import zignal_amd as zg
    return zg


SHAPES = {"aligned": (256, 512), "odd": (97, 131)}


def _dev_buffer(a: np.ndarray, layout: str):
    """A device buffer for host array `a`: contiguous ("aligned"), or a view one row and three columns into a larger parent ("odd")."""
    t = _torch()
    if layout != "view":
        return t.from_numpy(np.ascontiguousarray(a)).cuda()
    parent = t.zeros((a.shape[0] + 2, a.shape[1] + 5) + a.shape[2:], dtype=t.from_numpy(a[:1, :1]).dtype, device="cuda")
    v = parent[1:1 + a.shape[0], 3:3 + a.shape[1]]
    v.copy_(t.from_numpy(np.ascontiguousarray(a)))
    return v


def _sentinel(t):
    if t.dtype == torch.float32:
        t.fill_(float("nan"))
    elif t.dtype == torch.uint8:
        t.fill_(0xA5)
    else:
        t.fill_(-1)


def _bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got: np.ndarray, want: np.ndarray, what: str):
    from tests.util import assert_bits_equal
    assert_bits_equal(np.ascontiguousarray(got), np.ascontiguousarray(want), what)


class Capture:
    """zg_graph_begin/end_capture around a block on a side stream; the block's Image calls land on that stream."""

    def __init__(self):
        self.lib = _zg().lib()
        self.stream = torch.cuda.Stream()
        self.sp = C.c_void_p(self.stream.cuda_stream)
        self.graph = None

    def record(self, fn):
        torch.cuda.synchronize()
        g = C.c_void_p()
        with torch.cuda.stream(self.stream):
            assert self.lib.zg_graph_begin_capture(self.sp) == 0, self.lib.zg_last_error()
            try:
                fn()
            finally:
                rc = self.lib.zg_graph_end_capture(self.sp, C.byref(g))
        assert rc == 0, self.lib.zg_last_error()
        self.graph = g
        return self

    def launch(self):
        assert self.lib.zg_graph_launch(self.graph, self.sp) == 0, self.lib.zg_last_error()
        self.stream.synchronize()

    def destroy(self):
        if self.graph is not None:
            assert self.lib.zg_graph_destroy(self.graph) == 0
            self.graph = None


def replay_check(frames, setup, want, what, inplace=False, layout="aligned"):
    """frames: [A, B, C], each a list of host input arrays. setup(dev_inputs) -> (call, outputs); want(host_inputs) -> list of arrays
    (the outputs, or for an in-place op the inputs after the call)."""
    ins = [_dev_buffer(a, layout) for a in frames[0]]
    call, outs = setup(ins)
    torch.cuda.synchronize()  # the buffers were made on the default stream; everything below runs on the capture stream
    checked = ins if inplace else outs
    wants = [want([x.copy() for x in f]) for f in frames]
    assert any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(wants[0], wants[1])), f"{what}: A and B give the same result"
    cap = Capture()

    def load(f):
        for t, a in zip(ins, f):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        for o in outs:
            if not inplace:
                _sentinel(o)

    with torch.cuda.stream(cap.stream):
        load(frames[0])
        call()  # eager warm-up: first-use tables, scratch
    cap.stream.synchronize()
    with torch.cuda.stream(cap.stream):
        load(frames[0])
    cap.record(call)
    try:
        for k in (1, 2, 0):
            with torch.cuda.stream(cap.stream):
                load(frames[k])
            cap.launch()
            for i, (o, w) in enumerate(zip(checked, wants[k])):
                _same(o.cpu().numpy(), w, f"{what}: replay on input {'ABC'[k]}, output {i}")
    finally:
        cap.destroy()


def _img(t):
    return _zg().Image(t)


def _like(a_shape, dtype):
    return torch.empty(a_shape, dtype=dtype, device="cuda")


def _three(make):
    return [make(1), make(2), make(3)]


def _synth(o, kind, seed, shape):
    from tests.util import synth
    return synth(o, kind, seed, *shape)


def _canny_frames(shape):
    """A spiral of one weak stroke lit from one strong end (hysteresis across the whole frame), noise, and a flat frame."""
    r, c = shape
    spiral = np.zeros(shape, np.uint8)
    r0, r1, c0, c1 = 4, r - 5, 4, c - 5
    while r1 - r0 > 16 and c1 - c0 > 16:
        spiral[r0, c0:c1] = 40; spiral[r0:r1, c1] = 40; spiral[r1, c0 + 8:c1 + 1] = 40; spiral[r0 + 8:r1 + 1, c0 + 8] = 40
        r0 += 8; c0 += 8; r1 -= 8; c1 -= 8
    spiral[4, 4:12] = 255
    noise = np.random.default_rng(7).integers(0, 256, shape, dtype=np.uint8)
    flat = np.full(shape, 77, np.uint8)
    return spiral, noise, flat


def _bimodal(seed, shape, lo, hi):
    rng = np.random.default_rng(seed)
    a = rng.normal(lo, 12, shape)
    mask = rng.random(shape) < 0.4
    a[mask] = rng.normal(hi, 20, int(mask.sum()))
    return np.clip(a, 0, 255).astype(np.uint8)


def _skewed(seed, shape):
    """Histograms of different shapes: a narrow dark band, a ramp with an outlier tail, a wide mid-grey block."""
    rng = np.random.default_rng(seed)
    if seed == 1:
        return rng.integers(30, 70, shape, dtype=np.uint8)
    if seed == 2:
        a = (np.arange(shape[0] * shape[1]) % 200).reshape(shape[:2]).astype(np.uint8)
        a = np.ascontiguousarray(np.broadcast_to(a[..., None], shape) if len(shape) == 3 else a)
        a.reshape(-1)[:50] = 255
        return a
    return rng.integers(90, 250, shape, dtype=np.uint8)


def _row_cases():
    """(row name, pixel kind) pairs of the parametrised table test."""
    cases = []
    for name in ("conv_separable", "gaussian_blur", "convolve", "box_blur", "sharpen", "integral", "invert", "flips", "copy_fill_border",
                 "crop", "motion_linear", "motion_radial"):
        cases += [(name, k) for k in ("u8", "rgba_u8", "f32")]
    cases += [("resize", k) for k in ("u8", "f32", "rgb_u8", "rgba_u8", "rgb_f32", "rgba_f32")]
    for name in ("letterbox", "warp", "rotate_into", "extract", "insert", "convert", "resize_convert"):
        cases += [(name, k) for k in ("u8", "rgba_u8")]
    for name in ("order_statistic", "autocontrast", "equalize"):
        cases += [(name, k) for k in ("u8", "rgb_u8", "rgba_u8")]
    for name in ("conv_separable_planes", "gaussian_blur_planes", "devmath", "isef_smooth"):
        cases.append((name, "f32"))
    for name in ("sobel", "canny", "shen_castan", "morph", "threshold_otsu", "threshold_adaptive", "fast", "fast_batch", "pyramid_level",
                 "batch_blur_resize", "batch_pipeline"):
        cases.append((name, "u8" if name not in ("sobel", "batch_blur_resize", "batch_pipeline") else "rgba_u8"))
    return cases


METHOD_KINDS = ("nearest", "bilinear", "bicubic", "catmull_rom", "mitchell", "lanczos")


def _methods(zg):
    I = zg.Interpolation
    return {"nearest": I.nearest, "bilinear": I.bilinear, "bicubic": I.bicubic, "catmull_rom": I.catmull_rom,
            "mitchell": I.mitchell(1 / 3, 1 / 3), "lanczos": I.lanczos}


def _om(o, m):
    return o.method(m.kind, m.b, m.c)


def build_row(o, name, kind, shape):
    """frames, setup, want, inplace for one row."""
    zg = _zg()
    rows, cols = shape
    mk = lambda s: [_synth(o, kind, s, shape)]  # noqa: E731
    f32 = kind in ("f32", "rgb_f32", "rgba_f32")
    tdt = torch.float32 if f32 else torch.uint8
    ch = {"u8": (), "f32": (), "rgb_u8": (3,), "rgba_u8": (4,), "rgb_f32": (3,), "rgba_f32": (4,)}[kind]
    out_same = lambda ins: _like(tuple(ins[0].shape), tdt)  # noqa: E731

    def simple(op, oracle_fn):
        def setup(ins):
            out = out_same(ins)
            return (lambda: op(_img(ins[0]), _img(out))), [out]
        return _three(mk), setup, (lambda f: [oracle_fn(f[0])]), False

    def inplace(op, oracle_fn, make=None):
        def setup(ins):
            return (lambda: op(_img(ins[0]))), []
        return _three(make or mk), setup, (lambda f: [oracle_fn(f[0])]), True

    kx = np.array([0.05, 0.25, 0.4, 0.25, 0.05], np.float32)
    ky = np.array([0.1, 0.2, 0.4, 0.2, 0.1], np.float32)
    if name == "conv_separable":
        return simple(lambda s, d: s.convolve_separable(kx, ky, 1, out=d), lambda a: o.conv_separable(a, kx, ky, 1))
    if name == "gaussian_blur":
        return simple(lambda s, d: s.gaussian_blur(2.0, out=d), lambda a: o.gaussian_blur(a, 2.0))
    if name == "convolve":
        k = np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]], np.float32) / 1.5
        return simple(lambda s, d: s.convolve(k, 2, out=d), lambda a: o.convolve(a, k, 2))
    if name == "box_blur":
        return simple(lambda s, d: s.box_blur(3, out=d), lambda a: o.box_blur(a, 3))
    if name == "sharpen":
        return simple(lambda s, d: s.sharpen(2, out=d), lambda a: o.sharpen(a, 2))
    if name == "integral":
        nch = 1 if not ch else ch[0]

        def setup(ins):
            planes = _like((nch, rows, cols), torch.float32)
            lib = zg.lib()

            def call():
                d = _img(ins[0])._desc()
                assert lib.zg_integral(C.byref(d), C.cast(C.c_void_p(planes.data_ptr()), C.POINTER(C.c_float)),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            return call, [planes]
        return _three(mk), setup, (lambda f: [o.integral(f[0])]), False
    if name == "invert":
        if kind == "f32":
            mk8 = lambda s: [_synth(o, "u8", s, shape)]  # noqa: E731  (Image(f32).invert is a compile error in the reference)
            return inplace(lambda i: i.invert(), o.invert, mk8)
        return inplace(lambda i: i.invert(), o.invert)
    if name == "flips":
        return inplace(lambda i: (i.flip_left_right(), i.flip_top_bottom()), lambda a: o.flip_top_bottom(o.flip_left_right(a)))
    if name == "copy_fill_border":
        val = 0.25 if f32 else 200
        pix = val if not ch else [val] * ch[0]

        def setup(ins):
            out = out_same(ins)
            return (lambda: (_img(ins[0]).copy(_img(out)), _img(out).view((20, 10, 40, 30)).fill(pix),
                             _img(out).set_border((5, 4, cols - 6, rows - 5), pix))), [out]

        def want(f):  # the copied frame, a filled patch inside it, a border around it
            a = f[0].copy()
            o.fill(a[10:30, 20:40], pix)
            o.set_border(a, (5, 4, cols - 6, rows - 5), pix)
            return [a]
        return _three(mk), setup, want, False
    if name == "crop":
        rect = (5.0, 3.0, 5.0 + cols // 2, 3.0 + rows // 2)
        return _crop_row(o, mk, rect, tdt)
    if name == "motion_linear":
        return simple(lambda s, d: s.motion_blur_linear(0.6, 7, out=d), lambda a: o.motion_blur_linear(a, 0.6, 7))
    if name == "motion_radial":
        return simple(lambda s, d: s.motion_blur_radial(0.4, 0.55, 0.5, False, out=d), lambda a: o.motion_blur_radial(a, 0.4, 0.55, 0.5, False))
    if name == "resize":
        ms = _methods(zg)

        def setup(ins):
            outs = [_like((rows * 2 // 3 + 1, cols * 3 // 2) + ch, tdt) for _ in ms]
            return (lambda: [_img(ins[0]).resize(_img(out), m) for out, m in zip(outs, ms.values())]), outs
        return _three(mk), setup, (lambda f: [o.resize(f[0], (rows * 2 // 3 + 1, cols * 3 // 2), _om(o, m)) for m in ms.values()]), False
    if name == "letterbox":
        m = zg.Interpolation.bilinear

        def setup(ins):
            out = _like((rows // 2 + 7, cols // 2 + 40) + ch, tdt)
            return (lambda: _img(ins[0]).letterbox(_img(out), m)), [out]

        def want(f):
            out = np.empty((rows // 2 + 7, cols // 2 + 40) + ch, f[0].dtype)
            o.letterbox(f[0], out, _om(o, m))
            return [out]
        return _three(mk), setup, want, False
    if name == "warp":
        H = [[0.9, 0.1, 4.0], [-0.05, 1.1, 2.0], [0.0002, 0.0001, 1.0]]

        def setup(ins):
            out = _like((rows - 9, cols - 13) + ch, tdt)
            return (lambda: _img(ins[0]).warp(zg.ProjectiveTransform(H), _img(out), zg.Interpolation.bicubic)), [out]
        return (_three(mk), setup, lambda f: [o.warp(f[0], (rows - 9, cols - 13), o.PROJECTIVE, np.array(H, np.float32), _om(o, zg.Interpolation.bicubic))],
                False)
    if name == "rotate_into":
        def setup(ins):
            out = _like((rows + 10, cols + 6) + ch, tdt)
            return (lambda: _img(ins[0]).rotate_into(_img(out), 0.3, zg.Interpolation.bilinear, 1)), [out]
        return (_three(mk), setup,
                lambda f: [o.rotate_into(f[0], np.empty((rows + 10, cols + 6) + ch, f[0].dtype), 0.3, _om(o, zg.Interpolation.bilinear), 1)], False)
    if name == "extract":
        rect = (10.0, 8.0, 10.0 + cols / 2, 8.0 + rows / 2)

        def setup(ins):
            out = _like((rows // 3, cols // 3) + ch, tdt)
            return (lambda: _img(ins[0]).extract(rect, 0.4, _img(out), zg.Interpolation.catmull_rom, 2)), [out]
        return (_three(mk), setup,
                lambda f: [o.extract(f[0], np.empty((rows // 3, cols // 3) + ch, f[0].dtype), rect, 0.4, _om(o, zg.Interpolation.catmull_rom), 2)],
                False)
    if name == "insert":
        rect = (7.0, 5.0, 7.0 + cols / 2, 5.0 + rows / 3)
        src_shape = (rows // 3, cols // 4)
        blend = 1 if kind == "rgba_u8" else 0
        mk2 = lambda s: [_synth(o, kind, s, shape), _synth(o, kind, s + 10, src_shape)]  # noqa: E731

        def setup(ins):
            return (lambda: _img(ins[0]).insert(_img(ins[1]), rect, 0.2, zg.Interpolation.bilinear, blend)), []
        return (_three(mk2), setup,
                lambda f: [o.insert(f[0], f[1], rect, 0.2, _om(o, zg.Interpolation.bilinear), blend), f[1]], True)
    if name == "convert":
        # u8 -> Oklab (the sRGB table), rgba -> grey u8
        space = zg.CS_GRAY if kind == "u8" else zg.CS_RGBA

        def setup(ins):
            a = _like((rows, cols, 3), torch.float32)
            b = _like((rows, cols), torch.uint8) if kind != "u8" else _like((rows, cols, 4), torch.uint8)
            dst2 = zg.CS_GRAY if kind != "u8" else zg.CS_RGBA
            return (lambda: (_img(ins[0]).convert(zg.CS_OKLAB, np.float32, src_space=space, out=_img(a)),
                             _img(ins[0]).convert(dst2, np.uint8, src_space=space, out=_img(b)))), [a, b]

        def want(f):
            dst2, ch2 = (zg.CS_GRAY, 1) if kind != "u8" else (zg.CS_RGBA, 4)
            return [o.convert(f[0], space, zg.CS_OKLAB, np.float32, 3), o.convert(f[0], space, dst2, np.uint8, ch2)]
        return _three(mk), setup, want, False
    if name == "resize_convert":
        space = zg.CS_GRAY if kind == "u8" else zg.CS_RGBA

        def setup(ins):
            out = _like((rows // 2, cols // 2, 3), torch.float32)
            return (lambda: _img(ins[0]).resize_convert(_img(out), zg.CS_OKLAB, np.float32, zg.Interpolation.bilinear, src_space=space)), [out]
        return (_three(mk), setup,
                lambda f: [o.convert(o.resize(f[0], (rows // 2, cols // 2), _om(o, zg.Interpolation.bilinear)), space, zg.CS_OKLAB, np.float32, 3)],
                False)
    if name in ("conv_separable_planes", "gaussian_blur_planes"):
        mk4 = lambda s: [_synth(o, "f32", s * 4 + p, shape) for p in range(4)]  # noqa: E731

        def setup(ins):
            outs = [_like((rows, cols), torch.float32) for _ in ins]
            if name == "gaussian_blur_planes":
                return (lambda: zg.gaussian_blur_planes([_img(t) for t in ins], 1.4, [_img(t) for t in outs])), outs
            return (lambda: zg.convolve_separable_planes([_img(t) for t in ins], kx, ky, 2, [_img(t) for t in outs])), outs
        if name == "gaussian_blur_planes":
            return _three(mk4), setup, (lambda f: [o.gaussian_blur(a, 1.4) for a in f]), False
        return _three(mk4), setup, (lambda f: [o.conv_separable(a, kx, ky, 2) for a in f]), False
    if name == "devmath":
        n = rows * cols
        mkv = lambda s: [np.random.default_rng(s).uniform(0.01, 3.0, (rows, cols)).astype(np.float32)]  # noqa: E731

        def setup(ins):
            outs = [_like((rows, cols), torch.float32) for _ in range(3)]
            lib = zg.lib()

            def call():
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                for fn, out in zip((0, 3, 8), outs):
                    assert lib.zg_devmath_apply(fn, C.c_void_p(ins[0].data_ptr()), None, C.c_void_p(out.data_ptr()), n, st) == 0
            return call, outs
        return _three(mkv), setup, (lambda f: _devmath_want(o, f[0])), False
    if name == "isef_smooth":
        return simple(lambda s, d: s.isef_smooth(0.8, out=d), lambda a: o.isef_plane(a, 0.8))
    if name == "sobel":
        def setup(ins):
            out = _like((rows, cols), torch.uint8)
            return (lambda: _img(ins[0]).sobel(out=_img(out))), [out]
        return _three(mk), setup, (lambda f: [o.sobel(f[0])]), False
    if name == "canny":
        sp, no, fl = _canny_frames(shape)

        def setup(ins):
            out = _like((rows, cols), torch.uint8)
            return (lambda: _img(ins[0]).canny(0.0, 20, 600, out=_img(out))), [out]
        return [[sp], [no], [fl]], setup, (lambda f: [o.canny(f[0], 0.0, 20, 600)]), False
    if name == "shen_castan":
        def setup(ins):
            out = _like((rows, cols), torch.uint8)
            return (lambda: _img(ins[0]).shen_castan(out=_img(out))), [out]
        sp, no, fl = _canny_frames(shape)
        return [[sp], [no], [fl]], setup, (lambda f: [o.shen_castan(f[0])]), False
    if name == "order_statistic":
        def setup(ins):
            outs = [out_same(ins) for _ in range(3)]
            return (lambda: (_img(ins[0]).median_blur(2, out=_img(outs[0])), _img(ins[0]).max_blur(1, 0, out=_img(outs[1])),
                             _img(ins[0]).alpha_trimmed_mean_blur(2, 0.2, 3, out=_img(outs[2])))), outs
        return (_three(mk), setup, lambda f: [o.order_statistic_blur(f[0], 2, 0, 0.5, 2), o.order_statistic_blur(f[0], 1, 0, 1.0, 0),
                                               o.order_statistic_blur(f[0], 2, 2, 0.2, 3)], False)
    if name == "morph":
        k = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
        mkb = lambda s: [np.where(_synth(o, "u8", s, shape) > 128 + 20 * s, 255, 0).astype(np.uint8)]  # noqa: E731

        def setup(ins):
            outs = [out_same(ins) for _ in range(4)]
            return (lambda: [getattr(_img(ins[0]), f)(k, 2, out=_img(out)) for f, out in
                             zip(("dilate_binary", "erode_binary", "open_binary", "close_binary"), outs)]), outs
        return _three(mkb), setup, (lambda f: [o.morph(f[0], k, 2, op) for op in range(4)]), False
    if name == "threshold_otsu":
        mko = lambda s: [_bimodal(s, shape, 40 + 30 * s, 200 - 10 * s)]  # noqa: E731

        def setup(ins):
            out = out_same(ins)
            lib = zg.lib()

            def call():  # threshold_out NULL: the capturable form
                s, d = _img(ins[0])._desc(), _img(out)._desc()
                assert lib.zg_threshold_otsu(C.byref(s), C.byref(d), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            return call, [out]
        thresholds = {o.threshold_otsu(mko(s)[0])[1] for s in (1, 2, 3)}
        assert len(thresholds) == 3, thresholds
        return _three(mko), setup, (lambda f: [o.threshold_otsu(f[0])[0]]), False
    if name == "threshold_adaptive":
        return simple(lambda s, d: s.threshold_adaptive_mean(3, 2.0, out=d), lambda a: o.threshold_adaptive_mean(a, 3, 2.0))
    if name in ("autocontrast", "equalize"):
        mks = lambda s: [_skewed(s, shape + ch)]  # noqa: E731
        if name == "autocontrast":
            return inplace(lambda i: i.autocontrast(0.02), lambda a: o.autocontrast(a, 0.02), mks)
        return inplace(lambda i: i.equalize(), o.equalize, mks)
    if name in ("fast", "fast_batch"):
        return _fast_row(o, name, shape)
    if name == "pyramid_level":
        r2, c2, sig = _level_shape(zg, rows, cols, 1.5, 1.6, 1)

        def setup(ins):
            out = _like((r2, c2), torch.uint8)
            lib = zg.lib()

            def call():
                s, d = _img(ins[0])._desc(), _img(out)._desc()
                assert lib.zg_pyramid_build_level(C.byref(s), C.byref(d), C.c_float(sig), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            return call, [out]
        return _three(mk), setup, (lambda f: [o.pyramid(f[0], 2, 1.5, 1.6)[1]]), False
    if name == "batch_blur_resize":
        n = 3
        mkf = lambda s: [np.stack([_synth(o, kind, s * 10 + i, shape) for i in range(n)])]  # noqa: E731

        def setup(ins):
            out = _like((n, rows // 2, cols // 2) + ch, tdt)
            lib = zg.lib()
            m = zg.Interpolation.bilinear._c()

            def call():
                assert lib.zg_batch_blur_resize(C.c_void_p(ins[0].data_ptr()), n, rows, cols, 3, C.c_float(1.2), C.c_void_p(out.data_ptr()),
                                                rows // 2, cols // 2, C.byref(m), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            return call, [out]
        return (_three(mkf), setup,
                lambda f: [np.stack([o.resize(o.gaussian_blur(x, 1.2), (rows // 2, cols // 2), o.method(o.BILINEAR)) for x in f[0]])], False)
    if name == "batch_pipeline":
        return _pipeline_row(o, zg, shape)
    raise AssertionError(name)


def _crop_row(o, mk, rect, tdt):
    zg = _zg()
    want_shape = o.crop(mk(1)[0], rect).shape

    def setup(ins):
        out = _like(want_shape, tdt)
        return (lambda: _crop_into(zg, ins[0], out, rect)), [out]
    return _three(mk), setup, (lambda f: [o.crop(f[0], rect)]), False


def _crop_into(zg, src, out, rect):
    s, d = _img(src)._desc(), _img(out)._desc()
    assert zg.lib().zg_crop(C.byref(s), C.byref(d), (C.c_float * 4)(*rect), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0


def _devmath_want(o, x):
    """cbrt, log and gammaToLinear by the oracle's own maths (zo_math_apply, the reference tests/test_math_pin.py sweeps against)."""
    f = o.lib().zo_math_apply
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    x = np.ascontiguousarray(x, np.float32)
    outs = []
    for fn in (0, 3, 8):
        want = np.empty_like(x)
        assert f(fn, x.ctypes.data, None, want.ctypes.data, x.size) == 0
        outs.append(want)
    return outs


def _level_shape(zg, rows, cols, factor, sigma, level):
    lib = zg.lib()
    scale = lib.zg_pyramid_scale(C.c_float(factor), level)
    r, c, s = C.c_uint32(), C.c_uint32(), C.c_float()
    assert lib.zg_pyramid_level(rows, cols, C.c_float(scale), C.c_float(sigma), C.byref(r), C.byref(c), C.byref(s)) == 0
    return r.value, c.value, s.value


def _fast_row(o, name, shape):
    from tests import fast_ref as F
    zg = _zg()
    KP = zg.KEYPOINT_DTYPE.itemsize
    lib = zg.lib()
    # A: noise, many corners (more than the small buffer holds); B: a photo-like frame, few; C: flat, none
    mkf = {1: lambda: o.synth_u8(31, shape), 2: lambda: F.photo_like(o.synth_u8(32, shape)), 3: lambda: np.full(shape, 90, np.uint8)}
    frames = [[mkf[s]()] for s in (1, 2, 3)]
    caps = (5000, 7)

    def setup(ins):
        kps = [torch.zeros(c * KP, dtype=torch.uint8, device="cuda") for c in caps]
        counts = torch.zeros(len(caps), dtype=torch.int32, device="cuda")

        def call():
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            d = _img(ins[0])._desc()
            if name == "fast":
                for i, c in enumerate(caps):
                    assert lib.zg_fast_detect(C.byref(d), 20, 9, 1, C.c_void_p(kps[i].data_ptr()), c,
                                              C.c_void_p(counts.data_ptr() + 4 * i), st) == 0, lib.zg_last_error()
            else:
                whole = kps[0]  # both images' keypoints in one buffer: [0, 4000) and [4000, 4007)
                imgs = (L_img(zg) * 2)(d, d)
                assert lib.zg_fast_detect_batch(imgs, 2, (C.c_uint32 * 2)(20, 12), 9, 1, C.c_void_p(whole.data_ptr()), (C.c_uint32 * 2)(4000, 7),
                                                (C.c_uint64 * 2)(0, 4000), C.c_void_p(counts.data_ptr()), st) == 0, lib.zg_last_error()
        return call, [counts] + kps

    def want(f):
        img = f[0]
        if name == "fast":
            a, b = F.detect_fast(img, 20, 9, True), F.detect_fast(img, 20, 9, True)
            buf = np.full(caps[0] * KP, 0xA5, np.uint8)  # past the list the buffer keeps the sentinel
            buf[:min(len(a), caps[0]) * KP] = a[:caps[0]].view(np.uint8).reshape(-1)
            small = np.full(caps[1] * KP, 0xA5, np.uint8)  # capacity below the count: the first 7 of the list, the full count
            small[:min(len(b), caps[1]) * KP] = b[:caps[1]].view(np.uint8).reshape(-1)
            return [np.array([len(a), len(b)], np.int32), buf, small]
        a, b = F.detect_fast(img, 20, 9, True), F.detect_fast(img, 12, 9, True)
        buf = np.full(caps[0] * KP, 0xA5, np.uint8)
        buf[:min(len(a), 4000) * KP] = a[:4000].view(np.uint8).reshape(-1)
        buf[4000 * KP:(4000 + min(len(b), 7)) * KP] = b[:7].view(np.uint8).reshape(-1)
        return [np.array([len(a), len(b)], np.int32), buf, np.full(caps[1] * KP, 0xA5, np.uint8)]

    assert len(F.detect_fast(frames[0][0], 20, 9, True)) > caps[1]
    return frames, setup, want, "fast"


def L_img(zg):
    from zignal_amd import _lib as L
    return L.ZgImage


def _pipeline_row(o, zg, shape):
    rows, cols = shape
    n = 2
    steps = [zg.Step.resize(rows * 3 // 4, cols * 3 // 4, zg.Interpolation.lanczos), zg.Step.gaussian_blur(2.0), zg.Step.edges_sobel()]
    pipe = zg.Pipeline(steps)
    mkf = lambda s: [np.stack([_synth(o, "rgba_u8", s * 10 + i, shape) for i in range(n)])]  # noqa: E731

    def setup(ins):
        out = _like((n, rows * 3 // 4, cols * 3 // 4, 4), torch.uint8)
        return (lambda: pipe.run(ins[0], out=out)), [out]

    def want(f):
        lan = o.method(o.LANCZOS)
        res = []
        for x in f[0]:
            g = o.gaussian_blur(o.resize(x, (rows * 3 // 4, cols * 3 // 4), lan), 2.0)
            grey = o.convert(g, zg.CS_RGBA, zg.CS_GRAY, np.uint8, 1)
            res.append(o.convert(o.sobel(grey), zg.CS_GRAY, zg.CS_RGBA, np.uint8, 4))
        return [np.stack(res)]
    return _three(mkf), setup, want, False


CASES = _row_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ("aligned", "view"))
@pytest.mark.parametrize("name,kind", CASES, ids=[f"{n}-{k}" for n, k in CASES])
def test_replay_on_changed_inputs(oracle, name, kind, layout):
    shape = SHAPES["aligned" if layout == "aligned" else "odd"]
    if layout == "view" and name in ("batch_blur_resize", "batch_pipeline", "conv_separable_planes", "gaussian_blur_planes", "devmath", "isef_smooth"):
        layout = "odd"  # contiguous frame batches, plane arrays and planes (isef_smooth): the odd shape is the fallback
    frames, setup, want, flag = build_row(oracle, name, kind, shape)
    replay_check(frames, setup, want, f"{name} {kind} {layout} {shape}", inplace=flag is True,
                 layout="view" if layout == "view" else "aligned")


# ---- beyond the table ----------------------------------------------------------------------------------------------------------------
def _lanczos(zg):
    return zg.Interpolation.lanczos


def _run_child(code, env_extra=None):
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                         env=dict(os.environ, **(env_extra or {})))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_torch_graph_capture_of_image_calls(oracle):
    """The Python layer's route: torch.cuda.graph (global capture mode) around Image calls, replayed on changed inputs."""
    zg = _zg()
    shape = (200, 328)
    host = [oracle.synth_u8(s, shape + (4,)) for s in (41, 42)]
    src = torch.from_numpy(host[0]).cuda()
    rs = torch.empty((150, 250, 4), dtype=torch.uint8, device="cuda")
    gb = torch.empty_like(src)
    cn = torch.empty(shape, dtype=torch.uint8, device="cuda")
    frames = torch.from_numpy(np.stack(host)).cuda()
    pipe = zg.Pipeline([zg.Step.resize(150, 246, _lanczos(zg)), zg.Step.gaussian_blur(2.0), zg.Step.edges_sobel()])
    pout = torch.empty((2, 150, 246, 4), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    holder = {}

    def calls():
        im = zg.Image(src)
        im.resize(zg.Image(rs), _lanczos(zg))
        im.gaussian_blur(2.0, out=zg.Image(gb))
        im.canny(1.0, 40, 120, out=zg.Image(cn))
        holder["pyr"] = zg.ImagePyramid.build(im, 4, 1.3, 1.6)
        pipe.run(frames, out=pout)

    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        calls()  # warm-up
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        calls()
    pyr = holder["pyr"]
    lan = oracle.method(oracle.LANCZOS)
    try:
        for k in (1, 0):
            a = oracle.synth_u8(43, shape + (4,)) if k else host[0]
            batch = np.stack([a, host[1]])
            src.copy_(torch.from_numpy(a))
            frames.copy_(torch.from_numpy(batch))
            for t in (rs, gb, cn, pout):
                _sentinel(t)
            for lv in pyr.levels[1:]:
                _sentinel(lv.data)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            _same(rs.cpu().numpy(), oracle.resize(a, (150, 250), lan), "torch graph: lanczos resize")
            _same(gb.cpu().numpy(), oracle.gaussian_blur(a, 2.0), "torch graph: gaussian")
            _same(cn.cpu().numpy(), oracle.canny(a, 1.0, 40, 120), "torch graph: canny")
            want_levels = oracle.pyramid(a, 4, 1.3, 1.6)[1:]
            assert len(want_levels) == len(pyr.levels) - 1
            for i, (lv, w) in enumerate(zip(pyr.levels[1:], want_levels)):
                _same(lv.to_numpy(), w, f"torch graph: pyramid level {i + 1}")
            for f in range(2):
                g = oracle.gaussian_blur(oracle.resize(batch[f], (150, 246), lan), 2.0)
                want = oracle.convert(oracle.sobel(oracle.convert(g, zg.CS_RGBA, zg.CS_GRAY, np.uint8, 1)), zg.CS_GRAY, zg.CS_RGBA, np.uint8, 4)
                _same(pout[f].cpu().numpy(), want, f"torch graph: pipeline frame {f}")
    finally:
        del graph
        torch.cuda.synchronize()
        zg.lib().zg_release_graph_scratch()


def _chain_oracle(o, a, shape2):
    lan = o.method(o.LANCZOS)
    r = o.resize(a, shape2, lan)
    g = o.gaussian_blur(r, 2.0)
    return [r, g, o.sobel(g), o.canny(g, 1.0, 30, 90)]


@pytest.mark.gpu
def test_chain_in_one_graph_and_two_graphs_on_shared_buffers(oracle):
    """resize(.lanczos) -> gaussian(2.0: two passes through a temp plane) -> sobel -> canny in ONE capture (scratch handed on inside it),
    and a second graph over the same buffers doing other work; replayed alternately (first, second, first)."""
    zg = _zg()
    shape, shape2 = (240, 320), (180, 260)
    host = [oracle.synth_u8(s, shape + (4,)) for s in (51, 52, 53)]
    src = torch.from_numpy(host[0]).cuda()
    r = torch.empty(shape2 + (4,), dtype=torch.uint8, device="cuda")
    g = torch.empty_like(r)
    sb = torch.empty(shape2, dtype=torch.uint8, device="cuda")
    cn = torch.empty_like(sb)
    outs = [r, g, sb, cn]

    def chain1():
        zg.Image(src).resize(zg.Image(r), _lanczos(zg))
        zg.Image(r).gaussian_blur(2.0, out=zg.Image(g))
        zg.Image(g).sobel(out=zg.Image(sb))
        zg.Image(g).canny(1.0, 30, 90, out=zg.Image(cn))

    def chain2():
        zg.Image(src).resize(zg.Image(r), zg.Interpolation.bilinear)
        zg.Image(r).box_blur(2, out=zg.Image(g))
        zg.Image(g).sobel(out=zg.Image(sb))
        zg.Image(g).canny(0.0, 30, 90, out=zg.Image(cn))

    def want1(a):
        return _chain_oracle(oracle, a, shape2)

    def want2(a):
        rr = oracle.resize(a, shape2, oracle.method(oracle.BILINEAR))
        bb = oracle.box_blur(rr, 2)
        return [rr, bb, oracle.sobel(bb), oracle.canny(bb, 0.0, 30, 90)]

    c1 = Capture()
    c2 = Capture()
    c2.stream, c2.sp = c1.stream, c1.sp
    torch.cuda.synchronize()
    with torch.cuda.stream(c1.stream):
        chain1()
        chain2()
    c1.stream.synchronize()
    c1.record(chain1)
    c2.record(chain2)
    try:
        for gi, (cap, want) in enumerate(((c1, want1), (c2, want2), (c1, want1))):
            for k in (1, 2, 0):
                with torch.cuda.stream(c1.stream):
                    src.copy_(torch.from_numpy(host[k]))
                    for t in outs:
                        _sentinel(t)
                cap.launch()
                for i, (t, w) in enumerate(zip(outs, want(host[k]))):
                    _same(t.cpu().numpy(), w, f"graph {gi} input {'ABC'[k]} output {i}")
    finally:
        c1.destroy()
        c2.destroy()


def _pyramid_case(oracle, kind, shape, n, factor, sigma, layout="aligned"):
    """zg_pyramid_build captured (the route that forks the levels over four streams), every level against the oracle on B, C, A."""
    zg = _zg()
    from zignal_amd import _lib as L
    lib = zg.lib()
    f32 = kind == "f32"
    ch = (4,) if kind == "rgba_u8" else ()
    tdt = torch.float32 if f32 else torch.uint8
    frames = [oracle.synth_f32(s, shape + ch) if f32 else oracle.synth_u8(s, shape + ch) for s in (61, 62, 63)]
    src = _dev_buffer(frames[0], layout)
    shapes = []
    for i in range(1, n):
        r, c, sg = _level_shape(zg, shape[0], shape[1], factor, sigma, i)
        if r < 8 or c < 8:
            break
        shapes.append((r, c, sg))
    levels = [torch.empty((r, c) + ch, dtype=tdt, device="cuda") for r, c, _ in shapes]
    sigmas = (C.c_float * len(shapes))(*[sg for _, _, sg in shapes])
    assert len(levels) >= 3
    torch.cuda.synchronize()

    def call():
        d = zg.Image(src)._desc()
        descs = (L.ZgImage * len(levels))(*[zg.Image(t)._desc() for t in levels])
        assert lib.zg_pyramid_build(C.byref(d), descs, sigmas, len(levels), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, \
            lib.zg_last_error()

    cap = Capture()
    with torch.cuda.stream(cap.stream):
        call()
    cap.stream.synchronize()
    cap.record(call)
    try:
        for k in (1, 2, 0):
            with torch.cuda.stream(cap.stream):
                src.copy_(torch.from_numpy(frames[k]))
                for t in levels:
                    _sentinel(t)
            cap.launch()
            want = oracle.pyramid(frames[k], len(levels) + 1, factor, sigma)[1:]
            assert len(want) == len(levels)
            for i, (t, w) in enumerate(zip(levels, want)):
                _same(t.cpu().numpy(), w, f"pyramid {kind} {shape} {layout}: level {i + 1} on input {'ABC'[k]}")
    finally:
        cap.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape,layout", [("u8", (512, 768), "aligned"), ("u8", (301, 457), "view"), ("f32", (256, 384), "aligned"),
                                               ("rgba_u8", (203, 317), "aligned")])
def test_pyramid_forked_route_every_level(oracle, kind, shape, layout):
    _pyramid_case(oracle, kind, shape, 6, 1.5, 1.6, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2304, 3072), (613, 997)])
def test_pyramid_orb_default_under_capture(oracle, shape):
    """ORB's default: 8 levels at scale factor 1.2, on one large and one odd shape."""
    _pyramid_case(oracle, "u8", shape, 8, 1.2, 1.6)


@pytest.mark.gpu
def test_pyramid_without_the_tile_kernel_under_capture():
    """ZIGNAL_HIP_NO_PYRAMID_TILE (read once per process): the forked route's fallback levels, in a child process."""
    _run_child("import sys; sys.path.insert(0, %r)\n"
               "from oracle import pyoracle as o; o.lib()\n"
               "from tests.test_gpu_graph_replay import _pyramid_case\n"
               "_pyramid_case(o, 'u8', (400, 600), 6, 1.3, 1.6)\n"
               "_pyramid_case(o, 'u8', (211, 333), 6, 1.3, 1.6, 'view')\n"
               "print('ok')\n" % ROOT, {"ZIGNAL_HIP_NO_PYRAMID_TILE": "1"})


SHEN_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from oracle import pyoracle as o
o.lib()
from tests.test_gpu_graph_replay import replay_check, _img, _like
rows, cols = 256, 1024
rng = np.random.default_rng(5)
smooth = np.full((rows, cols), 100, np.uint8)
smooth[:, cols // 2:] = 160
rough = smooth.copy()
rough[64:128, 200:600] = rng.integers(0, 256, (64, 400), dtype=np.uint8)
third = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
def setup(ins):
    out = _like((rows, cols), torch.uint8)
    return (lambda: _img(ins[0]).shen_castan(0.5, out=_img(out))), [out]
replay_check([[smooth], [rough], [third]], setup, lambda f: [o.shen_castan(f[0], 0.5)], "shen-castan, short warm-up")
# the plane test_next_rows.py drives the repair launch with (a rough block of values x 1e3 beside flat ones), against a flat plane
flat = np.full((rows, cols), 100.0, np.float32)
block = flat.copy()
block[64:128, 200:600] = rng.integers(0, 256, (64, 400)).astype(np.float32) * 1e3
block[200:, cols - 100:] = rng.random((rows - 200, 100), dtype=np.float32)
noise = rng.random((rows, cols), dtype=np.float32)
def setup_f(ins):
    out = _like((rows, cols), torch.float32)
    return (lambda: _img(ins[0]).isef_smooth(0.6, out=_img(out))), [out]
replay_check([[flat], [block], [noise]], setup_f, lambda f: [o.isef_plane(f[0], 0.6)], "isef, short warm-up")
print("ok")
"""


@pytest.mark.gpu
def test_shen_castan_repair_launch_under_replay():
    """ZIGNAL_HIP_ISEF_W=8 (read once) shortens the segments' warm-up, so whether a group's start passes its check, and whether the repair
    launch redoes it, depends on the pixels. That decision stays on the device: one graph must replay frames that decide differently.
    The frames follow test_next_rows.py's repair test (a rough block beside flat regions, where it found groups failing) plus a flat and
    a noise frame; which groups fail on each frame is not observed here."""
    _run_child(SHEN_CHILD % ROOT, {"ZIGNAL_HIP_ISEF_W": "8"})


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.gpu
def test_a_graph_keeps_the_lanczos_tables_it_points_at(oracle):
    """The Lanczos axis tables of Rgb(u8) / Rgba(u8) resizes live in an LRU of 64 geometries. A graph captured over one geometry must
    survive its eviction: 72 eager resizes of other geometries, then the replay is still bit-exact (the pipeline's resize step too)."""
    zg = _zg()
    lan = oracle.method(oracle.LANCZOS)
    srcs = {k: oracle.synth_u8(70 + k, (173, 219, k)) for k in (3, 4)}
    dev = {k: torch.from_numpy(v).cuda() for k, v in srcs.items()}
    outs = {k: torch.empty((131, 301, k), dtype=torch.uint8, device="cuda") for k in srcs}
    frames = torch.from_numpy(np.stack([srcs[4], srcs[4][::-1].copy()])).cuda()
    pipe = zg.Pipeline([zg.Step.resize(97, 157, _lanczos(zg)), zg.Step.gaussian_blur(1.0)])
    pout = torch.empty((2, 97, 157, 4), dtype=torch.uint8, device="cuda")

    def call():
        for k in srcs:
            zg.Image(dev[k]).resize(zg.Image(outs[k]), _lanczos(zg))
        pipe.run(frames, out=pout)

    cap = Capture()
    torch.cuda.synchronize()
    with torch.cuda.stream(cap.stream):
        call()
    cap.stream.synchronize()
    cap.record(call)
    try:
        small = torch.from_numpy(oracle.synth_u8(79, (40, 50, 4))).cuda()
        for i in range(72):  # distinct geometries: every table of the capture leaves the cache
            zg.Image(small).resize((23 + i, 61 + 2 * i), _lanczos(zg))
        torch.cuda.synchronize()
        new = {k: oracle.synth_u8(90 + k, (173, 219, k)) for k in srcs}
        with torch.cuda.stream(cap.stream):
            for k in srcs:
                dev[k].copy_(torch.from_numpy(new[k]))
                _sentinel(outs[k])
            frames.copy_(torch.from_numpy(np.stack([new[4], new[4][::-1].copy()])))
            _sentinel(pout)
        cap.launch()
        for k in srcs:
            _same(outs[k].cpu().numpy(), oracle.resize(new[k], (131, 301), lan), f"evicted table, {k} channels")
        for f, a in enumerate((new[4], new[4][::-1].copy())):
            _same(pout[f].cpu().numpy(), oracle.gaussian_blur(oracle.resize(a, (97, 157), lan), 1.0), f"evicted table, pipeline frame {f}")
    finally:
        cap.destroy()


@pytest.mark.gpu
def test_graphs_hold_their_tables_until_they_are_destroyed(oracle):
    """A graph keeps the Lanczos axis tables it points at, and gives them back: live graphs hold their tables after the cache has let
    them go; destroying the graphs (zg_graph_* captures) or releasing them (captures torch ended, zg_release_graph_scratch) returns the
    memory; 100 capture / destroy cycles leave nothing behind. The x tables are 48 B per destination column (6 taps, index and weight),
    about 4.8 MB here: a leak of the holds would keep some 480 MB, against a 16 MiB allowance for other users of the device's memory."""
    zg = _zg()
    lib = zg.lib()
    lan = _lanczos(zg)
    src = torch.from_numpy(oracle.synth_u8(80, (64, 400, 4))).cuda()
    out = torch.empty((8, 110000, 4), dtype=torch.uint8, device="cuda")
    tiny = torch.from_numpy(oracle.synth_u8(81, (16, 16, 4))).cuda()
    table = 48 * 100000  # allocations this large come straight from the driver, so free device memory shows them
    cap = Capture()

    def view(i):
        return zg.Image(out[:, :100000 + 7 * i])

    def capture(i):
        v = view(i)
        with torch.cuda.stream(cap.stream):
            zg.Image(src).resize(v, lan)  # the geometry's tables, cached eagerly
        cap.record(lambda: zg.Image(src).resize(v, lan))
        cap.launch()
        g, cap.graph = cap.graph, None
        return g

    def settled():  # 70 small geometries push every large table out of the cache's 64; then nothing idle is left anywhere
        for k in range(70):
            zg.Image(tiny).resize((5 + k % 7, 9 + k), lan)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        lib.zg_trim_scratch()
        return _free_bytes()

    assert lib.zg_graph_destroy(capture(0)) == 0
    base = settled()
    live = [capture(1 + i) for i in range(20)]
    held = base - settled()
    assert held >= 20 * table, f"20 live graphs hold {held} bytes, less than their tables"
    for g in live:
        assert lib.zg_graph_destroy(g) == 0
    assert base - settled() <= 16 * 2**20, "zg_graph_destroy did not give the tables back"
    for i in range(100):
        assert lib.zg_graph_destroy(capture(100 + i)) == 0
    assert base - settled() <= 16 * 2**20, "capture / destroy cycles leak"
    # captures that torch ends: their holds wait for zg_release_graph_scratch, called once the graphs are gone
    side = torch.cuda.Stream()
    graphs = []
    for i in range(10):
        v = view(400 + i)
        with torch.cuda.stream(side):
            zg.Image(src).resize(v, lan)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            zg.Image(src).resize(v, lan)
        graphs.append(g)
    del graphs, g
    torch.cuda.synchronize()
    before = settled()  # the graphs are gone, their holds are not
    assert lib.zg_release_graph_scratch() == 0
    freed = settled() - before
    assert freed >= 10 * table, f"zg_release_graph_scratch gave back {freed} bytes, less than 10 tables"


# ---- calls that cannot be captured: refused before they enqueue anything --------------------------------------------------------------
def _err(lib):
    e = lib.zg_last_error()
    return e.decode() if isinstance(e, bytes) else str(e)


def _refused_then_eager(lib, enqueue, eager_check, what):
    """enqueue(stream) under a zg capture must return ZG_ERR_UNSUPPORTED naming the capture; the capture still ends cleanly (its graph is
    destroyed, never launched) and the same call eagerly on the same stream is bit-exact."""
    cap = Capture()
    torch.cuda.synchronize()
    g = C.c_void_p()
    with torch.cuda.stream(cap.stream):
        assert lib.zg_graph_begin_capture(cap.sp) == 0
        try:
            rc = enqueue(cap.sp)
            msg = _err(lib)
        finally:
            end = lib.zg_graph_end_capture(cap.sp, C.byref(g))
    assert rc == UNSUPPORTED, f"{what}: status {rc} under capture ({msg})"
    assert "capturing" in msg and "graph" in msg, msg
    assert end == 0, f"{what}: the refusal invalidated the capture ({_err(lib)})"
    assert lib.zg_graph_destroy(g) == 0
    with torch.cuda.stream(cap.stream):
        assert enqueue(cap.sp) == 0, _err(lib)
    cap.stream.synchronize()
    eager_check()


@pytest.mark.gpu
def test_non_capturable_calls_refuse_and_leave_the_stream_usable(oracle):
    zg = _zg()
    from zignal_amd import _lib as L
    lib = zg.lib()
    F32P = C.POINTER(C.c_float)
    host = oracle.synth_u8(85, (60, 90, 4))
    src = torch.from_numpy(host).cuda()
    out = torch.empty_like(src)
    sd, od = zg.Image(src)._desc(), zg.Image(out)._desc()
    # warm the library's own tables first: these are the warm routes
    zg.Image(src).resize((30, 40), zg.Interpolation.lanczos)
    zg.Image(src).warp(zg.AffineTransform([[1.0, 0.0], [0.0, 1.0]], [0.0, 0.0]), (30, 40), zg.Interpolation.lanczos)
    zg.Image(src).convert(zg.CS_OKLAB, np.float32)
    torch.cuda.synchronize()

    # a caller's sRGB table
    slut = np.ascontiguousarray(oracle.srgb_to_linear_lut(), np.float32)
    ok = torch.empty((60, 90, 3), dtype=torch.float32, device="cuda")
    okd = zg.Image(ok)._desc()
    _refused_then_eager(lib, lambda st: lib.zg_convert(C.byref(sd), zg.CS_RGBA, C.byref(okd), zg.CS_OKLAB, slut.ctypes.data_as(F32P), st),
                        lambda: _same(ok.cpu().numpy(), oracle.convert(host, zg.CS_RGBA, zg.CS_OKLAB, np.float32, 3, srgb_lut=slut), "convert, caller's lut"),
                        "srgb_lut")
    # a caller's Lanczos table (an Rgba(u8) warp samples through it)
    lut = np.ascontiguousarray(zg_lanczos_lut(oracle), np.float32)
    m = L.ZgMethod(5, 0.0, 0.0, lut.ctypes.data)
    mat = (C.c_float * 6)(1.0, 0.1, -0.05, 1.0, 2.0, 1.0)
    om = oracle.method(oracle.LANCZOS)
    om.lanczos_lut = lut.ctypes.data
    _refused_then_eager(lib, lambda st: lib.zg_warp(C.byref(sd), C.byref(od), 1, mat, C.byref(m), st),
                        lambda: _same(out.cpu().numpy(), oracle.warp(host, (60, 90), oracle.AFFINE, np.array(list(mat), np.float32), om),
                                      "warp with a caller's lut"), "lanczos_lut")
    # zg_resize_lanczos_weights
    rd_t = torch.empty((40, 70, 4), dtype=torch.uint8, device="cuda")
    rd = zg.Image(rd_t)._desc()
    wx = np.ascontiguousarray(zg.lanczos_plane_weights(90, 70), np.float32)
    wy = np.ascontiguousarray(zg.lanczos_plane_weights(60, 40), np.float32)
    _refused_then_eager(lib, lambda st: lib.zg_resize_lanczos_weights(C.byref(sd), C.byref(rd), wx.ctypes.data_as(F32P), wy.ctypes.data_as(F32P), st),
                        lambda: _same(rd_t.cpu().numpy(), oracle.resize(host, (40, 70), oracle.method(oracle.LANCZOS)), "lanczos weights"),
                        "resize_lanczos_weights")
    # Otsu with threshold_out
    grey = _bimodal(4, (64, 96), 50, 190)
    gt = torch.from_numpy(grey).cuda()
    go = torch.empty_like(gt)
    gd, god = zg.Image(gt)._desc(), zg.Image(go)._desc()
    t = C.c_uint8(0)
    want_img, want_t = oracle.threshold_otsu(grey)

    def otsu_check():
        _same(go.cpu().numpy(), want_img, "otsu")
        assert t.value == want_t
    _refused_then_eager(lib, lambda st: lib.zg_threshold_otsu(C.byref(gd), C.byref(god), C.byref(t), st), otsu_check, "otsu threshold_out")
    # PNG decode
    png = oracle.png_encode_stored(host)
    pd_t = torch.empty_like(src)
    pdd = zg.Image(pd_t)._desc()
    buf = (C.c_uint8 * len(png)).from_buffer_copy(png)
    _refused_then_eager(lib, lambda st: lib.zg_png_decode(buf, len(png), None, C.byref(pdd), zg.CS_RGBA, None, st),
                        lambda: _same(pd_t.cpu().numpy(), host, "png decode"), "png decode")
    # an Rgba(u8) Lanczos geometry never resized before (its tables are not cached)
    nd_t = torch.empty((37, 53, 4), dtype=torch.uint8, device="cuda")
    ndd = zg.Image(nd_t)._desc()
    lm = zg.Interpolation.lanczos._c()
    _refused_then_eager(lib, lambda st: lib.zg_resize(C.byref(sd), C.byref(ndd), C.byref(lm), st),
                        lambda: _same(nd_t.cpu().numpy(), oracle.resize(host, (37, 53), oracle.method(oracle.LANCZOS)), "cold geometry"),
                        "uncached lanczos geometry")
    # a 2-D kernel larger than 15 x 15 (always the wide route, taps uploaded)
    k = ((np.arange(17 * 17, dtype=np.float32).reshape(17, 17) % 7) / 400.0).astype(np.float32)
    _refused_then_eager(lib, lambda st: lib.zg_convolve(C.byref(sd), C.byref(od), k.ctypes.data_as(F32P), 17, 17, 1, st),
                        lambda: _same(out.cpu().numpy(), oracle.convolve(host, k, 1), "convolve 17x17"), "convolve 17x17")
    # 301 taps on a 20 x 30 Rgb(f32) frame: its 360-byte rows are not 16-byte multiples, so the long-kernel f32 route declines and the
    # two-pass route, which uploads the taps, takes it
    rgbf = oracle.synth_f32(86, (20, 30, 3))
    rt = torch.from_numpy(rgbf).cuda()
    ro = torch.empty_like(rt)
    rtd, rod = zg.Image(rt)._desc(), zg.Image(ro)._desc()
    taps = np.full(301, 1.0 / 301, np.float32)
    _refused_then_eager(lib, lambda st: lib.zg_conv_separable(C.byref(rtd), C.byref(rod), taps.ctypes.data_as(F32P), 301, taps.ctypes.data_as(F32P),
                                                              301, 2, st),
                        lambda: _same(ro.cpu().numpy(), oracle.conv_separable(rgbf, taps, taps, 2), "separable 301 taps"), "separable 301 taps")
    # the synchronous copies
    hbuf = np.zeros(64, np.uint8)
    dbuf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    _refused_then_eager(lib, lambda st: lib.zg_memcpy_d2h(hbuf.ctypes.data, C.c_void_p(dbuf.data_ptr()), 64, st), lambda: None, "zg_memcpy_d2h")


def zg_lanczos_lut(oracle):
    """The 1025-entry Lanczos3 table as a caller would pass it: here the oracle's own values when it exports them, else f64 rounded."""
    if hasattr(oracle, "lanczos3_lut"):
        return oracle.lanczos3_lut()
    x = np.arange(1025, dtype=np.float64) * 3.0 / 1024.0
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(x == 0, 1.0, 3.0 * np.sin(np.pi * x) * np.sin(np.pi * x / 3.0) / (np.pi * np.pi * x * x))
    return v.astype(np.float32)


COLD_CHILD = """
import sys, ctypes as C
sys.path.insert(0, %r)
import numpy as np, torch
from oracle import pyoracle as o
o.lib()
import zignal_amd as zg
from tests.test_gpu_graph_replay import _refused_then_eager, _same
lib = zg.lib()
host = o.synth_u8(87, (50, 70))
src = torch.from_numpy(host).cuda()
out = torch.empty((31, 44), dtype=torch.uint8, device="cuda")
sd, od = zg.Image(src)._desc(), zg.Image(out)._desc()
m = zg.Interpolation.lanczos._c()
_refused_then_eager(lib, lambda st: lib.zg_resize(C.byref(sd), C.byref(od), C.byref(m), st),
                    lambda: _same(out.cpu().numpy(), o.resize(host, (31, 44), o.method(o.LANCZOS)), "first lanczos"), "first lanczos table")
rgba = o.synth_u8(88, (50, 70, 4))
rs = torch.from_numpy(rgba).cuda()
ok = torch.empty((50, 70, 3), dtype=torch.float32, device="cuda")
rsd, okd = zg.Image(rs)._desc(), zg.Image(ok)._desc()
_refused_then_eager(lib, lambda st: lib.zg_convert(C.byref(rsd), zg.CS_RGBA, C.byref(okd), zg.CS_OKLAB, None, st),
                    lambda: _same(ok.cpu().numpy(), o.convert(rgba, zg.CS_RGBA, zg.CS_OKLAB, np.float32, 3), "first srgb"), "first srgb table")
print("ok")
"""


@pytest.mark.gpu
def test_first_use_tables_refuse_under_capture_in_a_fresh_process():
    """A fresh process has neither the Lanczos table nor the sRGB table on the device: the first call that needs one is refused under
    capture (its upload cannot be recorded), the capture stays valid, and the same call eagerly afterwards is bit-exact."""
    _run_child(COLD_CHILD % ROOT)
