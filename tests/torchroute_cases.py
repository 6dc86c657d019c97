"""The case of tests/test_gpu_torchroute.py, in a child process (tests/torchroute.py).  python tests/torchroute_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import torch


def the_spin_measurement_tells_a_call_that_waits(rt, ctx):
    """returns_before_the_stream fails for a call that waits for the stream, and passes for one that does not touch it."""
    try:
        tr.returns_before_the_stream(torch.cuda.synchronize)
    except AssertionError:
        pass
    else:
        raise RuntimeError("a call that waits for the stream passed")
    torch.cuda.synchronize()
    tr.returns_before_the_stream(lambda: None)
    torch.cuda.synchronize()


if __name__ == "__main__":
    tr.main(globals())
