"""TEST INFRASTRUCTURE: operator cases of the fused inference convolution (mn_op_conv_bn_eval) that need a tile shape forced through
MN_HALO_A1 / MN_H2_HALO256, run in a process of their own (the library reads its knobs at the entry of every
mn_op_* call, csrc/knobs.h; a process of its own keeps a forced shape away from the other tests).  `python fused_eval_cases.py emu|hip`,
the group by FUSED_EVAL_GROUP = a1 | halo256.  Each case runs with and without a residual and with and without the ReLU
and prints its figures before it asserts."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

GROUPS = {"a1": ("MN_HALO_A1", "2", "A1_SHAPES"), "halo256": ("MN_H2_HALO256", "1", "HALO256_SHAPES")}


def main(backend):
    import fused_eval_checks as FE
    if backend == "emu":
        import emu_lib
        lib, dev = emu_lib.load(), "cpu"
    else:
        from geomapnet_amd import _binding
        lib, dev = _binding.hip(), "cuda"
    knob, value, shapes = GROUPS[os.environ["FUSED_EVAL_GROUP"]]
    assert os.environ.get(knob) == value, "%s=%s must be set for this group" % (knob, value)
    for shape in getattr(FE, shapes):
        FE.check_op(lib, dev, shape, log=print)
    print("fused-eval cases ok")


if __name__ == "__main__":
    main(sys.argv[1])
