"""zg_qr_detect under the conditions of tests/test_gpu_concurrency_tracer.py: two streams detecting in different frames at once, and eight
host threads inside the call at once, each with its own stream, frame and buffers. The scratch block of a call is a ScratchBlock on the
call's stream ([grey plane][binary map][workgroup counts][confirmed hits]); every expected result is computed serially before any
concurrent work starts, and every comparison is of bytes (tests/test_gpu_qr.py's check)."""
import threading

import pytest

torch = pytest.importorskip("torch")
from tests import qr_cases as K  # noqa: E402
from tests import qr_ref as R  # noqa: E402
from tests.test_gpu_qr import Out, check, dev, device_binary  # noqa: E402
from zignal_amd import qr  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("v1_axis", "v2_axis", "v7_axis", "v4_rot37", "v3_perspective", "tiled_finders", "tall_damaged", "all_light")


def test_two_streams_detect_in_different_frames_at_once():
    names = ("v10_axis", "tiled_finders")  # a long run of trials beside a long merge and 41 664 triples
    wants = [K.want(n) for n in names]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    frames = [dev(K.binary(n)) for n in names]
    outs = [Out() for _ in names]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, f, o in zip(streams, frames, outs):
            with torch.cuda.stream(s):
                o.run(f, qr.BINARY)
    torch.cuda.synchronize()
    for n, o, w in zip(names, outs, wants):
        check(n, o, w)


def test_eight_host_threads_inside_the_call():
    modes = [qr.BINARY if i % 2 == 0 else qr.OTSU for i in range(len(NAMES))]  # half of them through the threshold's scratch as well
    wants = [K.want(n) if m == qr.BINARY else R.detect(device_binary(K.frame(n), m)) for n, m in zip(NAMES, modes)]
    frames = [dev(K.binary(n) if m == qr.BINARY else K.frame(n)) for n, m in zip(NAMES, modes)]
    outs = [Out() for _ in NAMES]
    torch.cuda.synchronize()
    errors, barrier = [], threading.Barrier(len(NAMES))

    def work(i):
        try:
            stream = torch.cuda.Stream()
            barrier.wait()
            with torch.cuda.stream(stream):
                for _ in range(4):
                    outs[i].run(frames[i], modes[i])
            stream.synchronize()
        except Exception as e:  # noqa: BLE001
            errors.append((NAMES[i], repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(NAMES))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for n, o, w in zip(NAMES, outs, wants):
        check(n, o, w)
