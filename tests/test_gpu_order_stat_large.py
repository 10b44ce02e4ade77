"""Order-statistic blurs at radius 16..256 on the device (k_order_stat_hist, zignal_amd/csrc/order_stat.hip: a sliding 256-bin histogram per
lane, incremental rank trackers), bit for bit against oracle.order_statistic_blur, which evaluates every window directly. The oracle costs
(2r+1)^2 per sample, so the large radii go with tiny frames: a window larger than the frame only repeats border periods, which is where the
staging can go wrong. Every r >= 16 call answered ZG_ERR_UNSUPPORTED before this kernel existed."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import zignal_amd as zg  # noqa: E402
from tests import views  # noqa: E402
from tests.util import assert_bits_equal, synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("u8", "rgb_u8", "rgba_u8")
BORDERS = (0, 1, 2, 3)  # zero, replicate, mirror, wrap
PAIRS = ((0, 0.5), (0, 0.0), (0, 1.0), (0, 0.37), (1, 0.0), (2, 0.12), (2, 0.0), (2, 0.49))  # tests/test_next_rows.py:717
ALL = tuple((b, op, p) for b in BORDERS for op, p in PAIRS)


def dev(a):
    return zg.Image(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def run(img, radius, op, param, border):
    got = dev(img)._order_stat(radius, op, param, border, None)
    torch.cuda.synchronize()
    return got.to_numpy()


def check(oracle, img, radius, op, param, border, what):
    want = oracle.order_statistic_blur(img, radius, op, param, border)
    assert_bits_equal(run(img, radius, op, param, border), want, f"{what} r={radius} op={op} p={param} border={border}")


def rotating(start, count):
    """`count` of the 32 (border, op, param) pairings, from `start`, stepping by 5 (coprime to 32 and to 8: borders and pairs both rotate)."""
    return [ALL[(start + 5 * i) % len(ALL)] for i in range(count)]


def strip_rows(rows, radius, columns):
    """hist_strip_rows of order_stat.hip: rows per strip for a grid of `columns` workgroups per strip (column strips x channels)."""
    w = 2 * radius + 1
    n = min(max(rows // (4 * w), 1), -(-2048 // columns))
    if columns * n < 512:
        n = min(-(-512 // columns), max(rows // w, 1))
    return -(-rows // n)


@pytest.mark.parametrize("kind", KINDS)
def test_parity_at_radius_16(oracle, kind):
    """Every border with every (op, param) pair on 37x53; a rotating subset on 1x1, 3x3 (the window is larger than the frame: mirror and wrap
    periods repeat many times), 20x140 (three column strips, the last one ragged) and 70x9."""
    img = synth(oracle, kind, 128, 37, 53)
    for border, op, param in ALL:
        check(oracle, img, 16, op, param, border, f"{kind} 37x53")
    for k, (rows, cols) in enumerate(((1, 1), (3, 3), (20, 140), (70, 9))):
        img = synth(oracle, kind, 91 + rows, rows, cols)
        for border, op, param in rotating(7 * k + KINDS.index(kind), 8):
            check(oracle, img, 16, op, param, border, f"{kind} {rows}x{cols}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("radius", (17, 31))
def test_parity_at_radius_17_and_31(oracle, kind, radius):
    img = synth(oracle, kind, 200 + radius, 37, 53)
    for border, op, param in rotating(radius + 3 * KINDS.index(kind), 6):
        check(oracle, img, radius, op, param, border, f"{kind} 37x53")


def test_row_strip_seam(oracle):
    """A frame of 70 columns at r = 16 has two column strips; 100 rows are then cut into three row strips of H = 34, so rows 33|34 and 67|68
    are seams where a strip's first window is built from nothing, and 100 >= 2 H + 1."""
    rows = 100
    h = strip_rows(rows, 16, 2)
    assert h == 34 and rows >= 2 * h + 1
    img = synth(oracle, "u8", 77, rows, 70)
    check(oracle, img, 16, 0, 0.5, oracle.MIRROR, "seam median")
    check(oracle, img, 16, 2, 0.2, oracle.MIRROR, "seam trimmed")


def test_counter_width(oracle):
    """One bin holds the whole window: 65 025 at r = 127 (the largest count of a u16 counter) and 66 049 at r = 128 (u32 counters), on a
    constant frame under `replicate`; and bin 0 passes 65 535 at r = 128 on a 3x3 frame under `zero`."""
    const = np.full((3, 70), 255, np.uint8)
    noise = oracle.synth_u8(5, (3, 3))
    for op, param in ((0, 0.5), (1, 0.0), (2, 0.12)):
        for radius in (127, 128):
            check(oracle, const, radius, op, param, oracle.REPLICATE, "constant 255 3x70")
        check(oracle, noise, 128, op, param, oracle.ZERO, "noise 3x3")


def test_upper_bound(oracle):
    img = oracle.synth_u8(6, (5, 70))
    check(oracle, img, 256, 0, 0.5, oracle.MIRROR, "median 5x70")
    check(oracle, img, 256, 0, 1.0, oracle.WRAP, "max 5x70")
    with pytest.raises(zg.ZignalError) as e:
        dev(img).median_blur(257)
    assert e.value.status == zg._lib.ERR_UNSUPPORTED and "256" in str(e.value), str(e.value)
    with pytest.raises(zg.ZignalError):  # float pixels stay UnsupportedPixelType
        dev(np.zeros((4, 4), np.float32)).median_blur(16)


def test_adversarial_values(oracle):
    """A 0 / 255 checkerboard (the trackers cross the whole value range between neighbouring rows) and a horizontal ramp."""
    yy, xx = np.mgrid[0:37, 0:53]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)
    ramp = np.broadcast_to((np.arange(53) * 255 // 52).astype(np.uint8), (37, 53)).copy()
    for name, img in (("checkerboard", checker), ("ramp", ramp)):
        for op, param in ((0, 0.0), (0, 0.5), (0, 1.0), (1, 0.0), (2, 0.49)):
            for border in (oracle.MIRROR, oracle.ZERO):
                check(oracle, img, 16, op, param, border, name)


@pytest.mark.parametrize("kind", KINDS)
def test_views_and_aliasing(oracle, kind):
    img = synth(oracle, kind, 300, 37, 53)
    want_med = oracle.order_statistic_blur(img, 16, 0, 0.5, oracle.MIRROR)
    want_trim = oracle.order_statistic_blur(img, 16, 2, 0.2, oracle.WRAP)
    # source and destination views with stride > cols; nothing outside the destination view is written
    for placement in ("stride+1px" if kind != "rgba_u8" else "stride+4B", "origin+4B"):
        src = views.place(kind, 37, 53, placement).put(img)
        dst = views.place(kind, 37, 53, placement)
        src.image().median_blur(16, out=dst.image())
        assert_bits_equal(dst.take(f"median {kind} {placement}"), want_med, f"median into a view, {kind} {placement}")
        src.image().alpha_trimmed_mean_blur(16, 0.2, zg.BorderMode.wrap, out=dst.image())
        assert_bits_equal(dst.take(f"trimmed {kind} {placement}"), want_trim, f"trimmed into a view, {kind} {placement}")
        assert_bits_equal(src.take("source view"), img, "the source view is unchanged")
    # in place
    d = dev(img)
    d.median_blur(16, out=d)
    torch.cuda.synchronize()
    assert_bits_equal(d.to_numpy(), want_med, f"median in place {kind}")
    # a destination view that overlaps the source by a few rows
    ch = img.shape[2:]
    buf = torch.full((37 + 33, 53) + ch, 0xA5, dtype=torch.uint8, device="cuda")
    buf[33:].copy_(torch.from_numpy(img))
    zg.Image(buf[33:]).median_blur(16, out=zg.Image(buf[:37]))
    torch.cuda.synchronize()
    assert_bits_equal(buf[:37].cpu().numpy(), want_med, f"destination overlaps the source's first 4 rows, {kind}")
    assert_bits_equal(buf[37:].cpu().numpy(), img[4:], "the source rows below the destination are unchanged")


GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from oracle import pyoracle as o
o.lib()
import zignal_amd as zg
from tests.test_gpu_graph_replay import Capture
from tests.util import assert_bits_equal
hosts = [o.synth_u8(400 + i, (37, 53, 4)) for i in range(3)]
src = torch.from_numpy(hosts[0]).cuda()
med, trim = torch.empty_like(src), torch.empty_like(src)
cap = Capture()
# the first calls this process makes into the library are the captured ones
cap.record(lambda: (zg.Image(src).median_blur(16, out=zg.Image(med)), zg.Image(src).alpha_trimmed_mean_blur(16, 0.2, out=zg.Image(trim))))
for k in (1, 2):
    with torch.cuda.stream(cap.stream):
        src.copy_(torch.from_numpy(hosts[k]))
        med.fill_(0xA5)
        trim.fill_(0xA5)
    cap.launch()
    assert_bits_equal(med.cpu().numpy(), o.order_statistic_blur(hosts[k], 16, 0, 0.5, o.MIRROR), "replayed median %%d" %% k)
    assert_bits_equal(trim.cpu().numpy(), o.order_statistic_blur(hosts[k], 16, 2, 0.2, o.MIRROR), "replayed trimmed mean %%d" %% k)
cap.destroy()
print("ok")
"""


def _run_child(code, env_extra=None):
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, cwd=ROOT, env=dict(os.environ, **(env_extra or {})))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-3000:]  # one attempt: a failure is a failure


def test_graph_capture_as_the_first_work_of_a_process():
    """median_blur(16) and alpha_trimmed_mean_blur(16, 0.2) captured on one stream before the process has called the library for anything
    else, replayed twice on changed input."""
    _run_child(GRAPH_CHILD % ROOT)


def test_pipeline_median_steps(oracle):
    host = np.stack([oracle.synth_u8(500 + i, (24, 40, 4)) for i in range(3)])
    got = zg.Pipeline([zg.Step.median_blur(16)]).run(torch.from_numpy(host).cuda()).cpu().numpy()
    for f in range(3):
        assert_bits_equal(got[f], oracle.order_statistic_blur(host[f], 16, 0, 0.5), f"pipeline median 16, frame {f}")
    tiny = np.stack([oracle.synth_u8(510 + i, (3, 20)) for i in range(2)])
    got = zg.Pipeline([zg.Step.median_blur(256)]).run(torch.from_numpy(tiny).cuda()).cpu().numpy()
    for f in range(2):
        assert_bits_equal(got[f], oracle.order_statistic_blur(tiny[f], 256, 0, 0.5), f"pipeline median 256, frame {f}")
    with pytest.raises(zg.InvalidArgument):
        zg.Pipeline([zg.Step.median_blur(300)]).run(torch.from_numpy(host).cuda())


HOOK_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from oracle import pyoracle as o
o.lib()
import zignal_amd as zg
from tests.util import assert_bits_equal
pairs = %r
for shape, seed in (((37, 53, 4), 600), ((20, 140), 601)):
    img = o.synth_u8(seed, shape)
    d = zg.Image(torch.from_numpy(img).cuda())
    for radius in (1, 2, 4):
        for border in (0, 1, 2, 3):
            for op, param in pairs:
                got = d._order_stat(radius, op, param, border, None)
                torch.cuda.synchronize()
                assert_bits_equal(got.to_numpy(), o.order_statistic_blur(img, radius, op, param, border),
                                  "sliding kernel %%s r=%%d op=%%d p=%%s border=%%d" %% (shape, radius, op, param, border))
print("ok")
"""


def test_hook_runs_the_sliding_kernel_at_small_radii():
    """ZIGNAL_HIP_ORDER_STAT_HIST_MIN=1 sends every radius to the sliding kernel: r = 1, 2, 4, all borders, all eight (op, param) pairs."""
    _run_child(HOOK_CHILD % (ROOT, PAIRS), {"ZIGNAL_HIP_ORDER_STAT_HIST_MIN": "1"})
