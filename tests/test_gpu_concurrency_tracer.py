"""zg_trace_paths under the conditions of tests/test_gpu_concurrency_features.py: two streams tracing different frames at once, and eight
host threads inside the call at once, each with its own stream, frame and buffers. The scratch block of a call is a ScratchBlock on the
call's stream ([counts][columns][path records][queue][links][open][keep][labels][offsets][points][scan sums]); every expected list is
computed serially before any concurrent work starts, and every comparison is of bytes (tests/test_gpu_tracer.py's check)."""
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import zignal_amd as zg  # noqa: E402
from tests import tracer_cases as K  # noqa: E402
from tests.test_gpu_tracer import Out, check, dev, room  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("noise_0.3_0", "noise_0.45_1", "spiral_130", "junctions", "noise_0.6_2", "ring_130", "all_70x70", "noise_0.05_1")


def test_two_streams_trace_different_frames_at_once():
    names = ("noise_0.45_0", "serpentine_260")  # thousands of components beside one long walk
    wants = [K.want(n) for n in names]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    frames = [dev(K.frame(n)) for n in names]
    outs = [Out(*room(K.frame(n))) for n in names]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, f, o in zip(streams, frames, outs):
            with torch.cuda.stream(s):
                o.run(zg.Tracer(), f)
    torch.cuda.synchronize()
    for n, o, w in zip(names, outs, wants):
        check(n, o, w)


def test_eight_host_threads_inside_the_call():
    wants = [K.want(n) for n in NAMES]
    frames = [dev(K.frame(n)) for n in NAMES]
    outs = [Out(*room(K.frame(n))) for n in NAMES]
    torch.cuda.synchronize()
    errors, barrier = [], threading.Barrier(len(NAMES))

    def work(i):
        try:
            stream = torch.cuda.Stream()
            barrier.wait()
            with torch.cuda.stream(stream):
                for _ in range(4):
                    outs[i].run(zg.Tracer(), frames[i])
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
