"""The solo Adam kernels after the bias-correction memo (csrc/update_kernels.hip: adam_memo) still meet what
test_isa_cpu.py asks of the hot kernels: next to nothing in scratch memory, and the memo table -- a __device__ array read by
every workgroup -- reached by global loads, not flat ones.  Checked on the code objects inside the built library (no GPU)."""
import os

from recovery_rl_amd import _lib


def test_adam_kernels_stay_out_of_scratch_and_off_flat_loads(tmp_path):
    from isa_util import kernel_table
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    table = kernel_table(_lib.SO_PATH, str(tmp_path))
    for piece in ("adam_multi_kernel", "adam_multi_dual_kernel"):
        hits = {k: v for k, v in table.items() if piece in k and "vgpr" in v}
        assert len(hits) == 1, (piece, sorted(hits))
        for k, v in hits.items():
            assert v["scratch"] <= 32, (k, v["scratch"])
            assert v["vgpr"] <= 256, (k, v["vgpr"])              # two 4-wave workgroups per CU
            ins = v["ins"]
            assert not any(op.startswith("flat_load") for op in ins), (k, sorted(op for op in ins if op.startswith("flat")))
            assert not any(op.startswith("scratch_") for op in ins), k
            assert ins.get("global_load_dwordx4", 0) > 0
