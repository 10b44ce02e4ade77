"""zg_qr_detect and zg_canvas_cmds_from_qr on the device against tests/qr_ref.py, byte for byte: the detection record, the grid records
and the module bytes. The frames and what they are there for: tests/qr_cases.py; what stands behind the restatement:
tests/test_qr_oracle.py. Mode 2 (a binary map) isolates the detector from the threshold kernels; modes 0 and 1 run end to end, the
restatement then reads the map that Image.threshold_adaptive_mean / threshold_otsu (held to the reference by their own tests) produce."""
import ctypes as C

import numpy as np
import pytest

import zignal_amd as zg
from tests import canvas_cases as CK
from tests import canvas_ref as CR
from tests import qr_cases as K
from tests import qr_ref as R
from tests.canvas_cases import same_bytes
from zignal_amd import _lib as L
from zignal_amd import canvas, qr

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

GUARD, FILL = 64, 0x5A
DET, GRID = R.DETECTION_DTYPE.itemsize, R.GRID_DTYPE.itemsize
ROOM = (16, 16 * 3249)  # more grids and module bytes than any case here needs


class Out:
    """Device buffers for one detection with guard bytes behind all three, everything pre-filled with FILL."""

    def __init__(self, grid_capacity=ROOM[0], module_capacity=ROOM[1]):
        self.g_cap, self.m_cap = grid_capacity, module_capacity
        self.det = torch.full((DET + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.grids = torch.full((grid_capacity * GRID + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.modules = torch.full((module_capacity + GUARD,), FILL, dtype=torch.uint8, device="cuda")

    def run(self, image, mode):
        zg.QrDetector().detect_into(image, self.det, self.grids if self.g_cap else None, self.modules if self.m_cap else None, mode, self.g_cap, self.m_cap)
        return self

    def refill(self):
        for t in (self.det, self.grids, self.modules):
            t.fill_(FILL)

    def host(self):
        return tuple(t.cpu().numpy() for t in (self.det, self.grids, self.modules))


def check(name, out, want):
    """`out` against the restatement's result under the capacity rule: only whole grids, stopping at the first that does not fit."""
    det, grids, modules = out.host()
    w_det, w_grids, w_modules = R.pack(want, out.g_cap, out.m_cap)
    got = det[:DET].view(R.DETECTION_DTYPE)[0]
    for field in R.DETECTION_DTYPE.names:  # field by field first: a failure then names the stage
        assert got[field].tobytes() == w_det[field].tobytes(), f"{name}: detection.{field}: {got[field]} != {w_det[field]}"
    assert det[:DET].tobytes() == w_det.tobytes(), name
    n = len(w_grids)
    got_grids = grids[:n * GRID].view(R.GRID_DTYPE)
    for i in range(n):
        for field in R.GRID_DTYPE.names:
            assert got_grids[i][field].tobytes() == w_grids[i][field].tobytes(), f"{name}: grid {i}.{field}: {got_grids[i][field]} != {w_grids[i][field]}"
    assert grids[:n * GRID].tobytes() == w_grids.tobytes(), name
    assert modules[:len(w_modules)].tobytes() == w_modules.tobytes(), f"{name}: modules"
    assert (det[DET:] == FILL).all() and (grids[n * GRID:] == FILL).all() and (modules[len(w_modules):] == FILL).all(), f"{name}: written past the lists"


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cases are read-only


def same_grids(got, want, mode):
    assert len(got) == len(want["grids"])
    for g, w in zip(got, want["grids"]):
        assert (g.binarize, g.version, g.fourth_index, g.version_hint) == (mode, w["version"], w["fourth_index"], w["version_hint"])
        assert g.corners.tobytes() == w["corners"].tobytes() and g.transform.tobytes() == w["transform"].tobytes() and g.modules.tobytes() == w["modules"].tobytes()


# ---- the cases were fixed with the restatement on the CPU ------------------------------------------------------------------------------
def test_the_cases_reach_every_stage():
    wants = {name: K.want(name) for name in K.CASES}
    assert R.UNDEFINED_CASTS[0] == 0
    assert sum(len(w["grids"]) >= 1 for w in wants.values()) >= 8 and sum(len(w["grids"]) > 1 for w in wants.values()) >= 2
    assert wants["v1_axis"]["fourths"][-1][2] is False and len(wants["v1_axis"]["fourths"]) == 1  # no alignment pattern
    assert any(f[2] for f in wants["v2_axis"]["fourths"])
    assert [g["version_hint"] for g in wants["v7_axis"]["grids"]][:1] == [7] and [g["version_hint"] for g in wants["v10_axis"]["grids"]][:1] == [10]
    assert wants["tall_damaged"]["consumed"] and len(wants["tall_damaged"]["grids"]) >= 1  # the residue-1 and -2 passes were needed
    assert not wants["tall_undamaged"]["consumed"] and len(wants["tall_undamaged"]["grids"]) >= 1
    tiled = wants["tiled_finders"]
    assert tiled["merged_count"] == 64 and tiled["triple"] is not None and max(f[3] for f in tiled["finders"]) > 1
    assert len(wants["uncut_corner"]["grids"]) >= 1 and len(wants["cut_corner"]["grids"]) == 0 and wants["cut_corner"]["triple"] is not None
    for name in ("frame_20x40", "all_light", "all_dark"):
        assert wants[name]["merged_count"] == 0
    assert K.frame("frame_21").shape == (21, 21) and K.frame("frame_20x40").shape == (20, 40)


# ---- every frame as a binary map -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(K.CASES))
def test_binary_maps_equal_the_restatement(name):
    binary, want = K.binary(name), K.want(name)
    check(name, Out().run(dev(binary), qr.BINARY), want)
    if binary.size <= 120 * 120 or name in ("v7_axis", "v3_perspective"):  # the host form and the two-call wrapper, on both kinds of memory
        for image in (np.array(binary), dev(binary)):
            record, grids = zg.QrDetector().detect_pass(image, qr.BINARY)
            assert record.tobytes() == R.pack(want)[0].tobytes(), name
            same_grids(grids, want, qr.BINARY)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def device_binary(gray, mode):
    """What the reference's two thresholds give (detector.zig:73-79), by the library's own operations."""
    image = zg.Image(dev(gray))
    rows, cols = gray.shape
    out = image.threshold_adaptive_mean(max(min(rows, cols) // 16, 8), 4.0) if mode == qr.ADAPTIVE else image.threshold_otsu()
    out = out[0] if isinstance(out, tuple) else out
    return out.to_numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("v1_axis", "v2_axis", "v7_axis", "v4_rot37", "v3_perspective", "v5_gradient_noise", "tall_damaged"))
@pytest.mark.parametrize("mode", (qr.ADAPTIVE, qr.OTSU))
def test_grey_frames_end_to_end(name, mode):
    gray = K.frame(name)
    want = R.detect(device_binary(gray, mode))
    assert R.UNDEFINED_CASTS[0] == 0
    check(f"{name} mode {mode}", Out().run(dev(gray), mode), want)


@pytest.mark.gpu
def test_detect_returns_both_passes_tagged():
    gray = K.frame("v5_gradient_noise")
    wants = [R.detect(device_binary(gray, mode)) for mode in (qr.ADAPTIVE, qr.OTSU)]
    assert sum(len(w["grids"]) for w in wants) >= 1
    for image in (np.array(gray), dev(gray)):
        got = zg.QrDetector().detect(image)
        n0 = len(wants[0]["grids"])
        same_grids(got[:n0], wants[0], qr.ADAPTIVE)
        same_grids(got[n0:], wants[1], qr.OTSU)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", (3, 4))
def test_colour_sources_are_converted_first(channels):
    gray = K.frame("v2_axis")
    rng = np.random.default_rng(channels)
    rgb = np.clip(gray[..., None].astype(np.int64) + rng.integers(-25, 26, gray.shape + (3,)), 0, 255).astype(np.uint8)
    src = rgb if channels == 3 else np.concatenate((rgb, np.full(gray.shape + (1,), 255, np.uint8)), axis=2)
    as_u8 = zg.Image(dev(src)).convert(zg.CS_GRAY, np.uint8).to_numpy()  # Image.convert(u8), detector.zig:52
    for mode in (qr.ADAPTIVE, qr.OTSU):
        want = R.detect(device_binary(as_u8, mode))
        assert len(want["grids"]) >= 1
        check(f"{channels} channels mode {mode}", Out().run(dev(src), mode), want)
    out = Out()
    d = zg.Image(dev(src))._desc()
    assert zg.lib().zg_qr_detect(C.byref(d), qr.BINARY, C.c_void_p(out.det.data_ptr()), None, 0, None, 0, None) == L.ERR_UNSUPPORTED


# ---- views -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_window_of_a_larger_frame_and_a_padded_stride():
    name = "v2_axis"
    inner, want = K.binary(name), K.want(name)
    rows, cols = inner.shape
    big = torch.zeros((rows + 9, cols + 14), dtype=torch.uint8, device="cuda")  # dark all around: a walk that left the view would go on
    big[4:4 + rows, 5:5 + cols] = dev(inner)
    before = big.clone()
    check("window", Out().run(big[4:4 + rows, 5:5 + cols], qr.BINARY), want)
    assert torch.equal(big, before)
    padded = torch.zeros((rows, cols + 3), dtype=torch.uint8, device="cuda")
    padded[:, :cols] = dev(inner)
    check("stride", Out().run(padded[:, :cols], qr.BINARY), want)
    gray = K.frame(name)
    pad_gray = torch.full((rows + 2, cols + 5), 0, dtype=torch.uint8, device="cuda")
    pad_gray[1:1 + rows, 2:2 + cols] = dev(gray)
    before = pad_gray.clone()
    check("grey window", Out().run(pad_gray[1:1 + rows, 2:2 + cols], qr.OTSU), R.detect(device_binary(gray, qr.OTSU)))
    assert torch.equal(pad_gray, before)
    host = np.zeros((rows + 2, cols + 3), np.uint8)
    host[1:1 + rows, :cols] = inner
    record, grids = zg.QrDetector().detect_pass(host[1:1 + rows, :cols], qr.BINARY)
    same_grids(grids, want, qr.BINARY)


# ---- capacity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capacities_stop_at_whole_grids_and_report_the_full_need():
    name = "v7_axis"
    want = K.want(name)
    d = dev(K.binary(name))
    n = len(want["grids"])
    need = sum(g["dim"] ** 2 for g in want["grids"])
    first = want["grids"][0]["dim"] ** 2
    assert n >= 2
    for g_cap, m_cap in ((n, need), (n - 1, need), (n, need - 1), (n, first), (n, first - 1), (0, need), (n, 0), (0, 0), (1, need), (n + 3, need + 100)):
        out = Out(g_cap, m_cap).run(d, qr.BINARY)
        check(f"capacities {g_cap} {m_cap}", out, want)
        record = out.host()[0][:DET].view(R.DETECTION_DTYPE)[0]
        assert int(record["grids_total"]) == n and int(record["version_count"]) == len(want["versions"])
    det = L.ZgQrDetection()
    host_image = zg.Image(np.array(K.binary(name)))  # kept alive: the descriptor points into it
    desc = host_image._desc()
    assert zg.lib().zg_qr_detect_host(C.byref(desc), qr.BINARY, C.byref(det), None, 0, None, 0) == 0  # the counts alone
    assert (det.grids_total, det.grids_written, det.modules_written) == (n, 0, 0)


# ---- the builder ---------------------------------------------------------------------------------------------------------------------------
def outline(want, color, width, mode):
    cmds = []
    for g in want["grids"]:
        c = g["corners"].reshape(4, 2)
        ring = (c[0], c[1], c[3], c[2], c[0])
        cmds += [CK.line(float(a[0]), float(a[1]), float(b[0]), float(b[1]), color, width, mode) for a, b in zip(ring[:-1], ring[1:])]
    return cmds


@pytest.mark.gpu
def test_builder_outlines_the_corners_and_the_outline_is_drawn_on_the_frame():
    name = "v3_perspective"
    want = K.want(name)
    out = Out().run(dev(K.binary(name)), qr.BINARY)
    color = (255, 40, 10, 255)
    commands = outline(want, color, 1, CR.FAST)
    assert len(commands) == 4 * len(want["grids"]) >= 8
    cmds, count = canvas.cmds_from_qr(out.grids[:out.g_cap * GRID], out.det, color, 1, "fast")
    frame_host = np.repeat(K.frame(name)[..., None], 3, axis=2)
    frame = dev(frame_host)
    canvas.draw(frame, cmds, count=count)
    torch.cuda.synchronize()
    assert int(count.item()) == len(commands)
    assert cmds.cpu().numpy()[:len(commands) * 40].tobytes() == canvas.pack_commands(commands)[0].tobytes()
    assert same_bytes(frame.cpu().numpy(), CR.run(frame_host, commands))
    cap = len(commands) - 3  # a list shorter than the edges: the first `cap` of them, and nothing behind
    small = torch.full(((cap + 2) * 40,), 0x77, dtype=torch.uint8, device="cuda")
    _, count2 = canvas.cmds_from_qr(out.grids[:out.g_cap * GRID], out.det, color, 1, "fast", cmds_out=small[:cap * 40])
    got = small.cpu().numpy()
    assert int(count2.item()) == cap and got[:cap * 40].tobytes() == canvas.pack_commands(commands[:cap])[0].tobytes() and (got[cap * 40:] == 0x77).all()


# ---- graph ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_detect_then_draw_replays_from_a_graph_on_changed_frames():
    names = ("v2_axis", "all_light", "v1_axis")
    shape = K.frame("v2_axis").shape
    frames = {}
    for name in names:  # every frame on the first one's canvas
        f = np.full(shape, K.LIGHT, np.uint8)
        src = K.frame(name)
        r, c = min(shape[0], src.shape[0]), min(shape[1], src.shape[1])
        f[:r, :c] = src[:r, :c]
        frames[name] = f
    src = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    out = Out()
    cmds = torch.zeros(ROOM[0] * 4 * 40, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    drawn = torch.zeros(shape + (3,), dtype=torch.uint8, device="cuda")
    color = (0, 255, 0, 255)

    def enqueue():
        out.run(src, qr.OTSU)
        canvas.cmds_from_qr(out.grids[:out.g_cap * GRID], out.det, color, 1, "fast", cmds_out=cmds, count_out=count)
        drawn.zero_()
        canvas.draw(drawn, cmds, count=count)

    def verify(name, label):
        want = R.detect(device_binary(frames[name], qr.OTSU))
        check(label, out, want)
        commands = outline(want, color, 1, CR.FAST)
        assert int(count.item()) == len(commands), label
        assert same_bytes(drawn.cpu().numpy(), CR.run(np.zeros(shape + (3,), np.uint8), commands)), label
        return len(want["grids"])

    side = torch.cuda.Stream()
    src.copy_(dev(frames["v2_axis"]))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()  # captured before any eager call of the detector in this test
    with torch.cuda.graph(graph, stream=side):
        enqueue()
    seen = []
    for name in names:
        src.copy_(dev(frames[name]))
        out.refill()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        seen.append(verify(name, f"replay on {name}"))
    assert seen[0] >= 1 and seen[1] == 0 and seen[2] >= 1
    del graph
    torch.cuda.synchronize()
    assert zg.lib().zg_release_graph_scratch() == 0


# ---- status codes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_status_codes_are_decided_before_anything_is_enqueued():
    lib = zg.lib()
    binary = dev(K.binary("v1_axis"))
    out = Out(4, 4000)
    args = (C.c_void_p(out.det.data_ptr()), C.c_void_p(out.grids.data_ptr()), 4, C.c_void_p(out.modules.data_ptr()), 4000, None)
    d = zg.Image(binary)._desc()
    huge = zg.Image(binary)._desc()  # the descriptor alone: nothing of that size is allocated, and nothing is read
    huge.rows, huge.cols, huge.stride = 1 << 16, 1 << 15, 1 << 15
    assert lib.zg_qr_detect(C.byref(huge), qr.BINARY, *args) == L.ERR_UNSUPPORTED
    assert b"2^31" in lib.zg_last_error()
    assert lib.zg_qr_detect(None, qr.BINARY, *args) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_qr_detect(C.byref(d), 3, *args) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_qr_detect(C.byref(d), -1, *args) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_qr_detect(C.byref(d), qr.BINARY, None, *args[1:]) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_qr_detect(C.byref(d), qr.BINARY, args[0], None, 4, args[3], 4000, None) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_qr_detect(C.byref(d), qr.BINARY, args[0], args[1], 4, None, 4000, None) == L.ERR_INVALID_ARGUMENT
    col = (C.c_uint8 * 4)(1, 2, 3, 255)
    cmds, count = torch.zeros(40 * 16, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    good = (args[1], args[0], 16, col, 1, 0, C.c_void_p(cmds.data_ptr()), C.c_void_p(count.data_ptr()), None)
    for i, bad in ((0, None), (1, None), (3, None), (4, 1 << 20), (5, 7), (6, None), (7, None)):
        a = list(good)
        a[i] = bad
        assert lib.zg_canvas_cmds_from_qr(*a) == L.ERR_INVALID_ARGUMENT, i
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in (out.det, out.grids, out.modules))  # nothing ran
    assert qr.scratch_bytes(1080, 1920) == lib.zg_qr_scratch_bytes(1080, 1920) > 6 * 1080 * 1920
    assert qr.scratch_bytes(20, 40) == 0
