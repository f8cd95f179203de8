"""ISA lint of rs_bfinish_kernel, the bounded second pass's finish (CPU test: hipcc cross-compiles gfx950 to assembly here).

The finish is rs_score32_kernel's body under another kernel (rs_score32_body<false, true>, ransac.hip), so it carries the same
inline-asm `s_load_dwordx16` prefetch of the fp32 rows with the wait in a separate asm statement, and the same rule holds for it:
no instruction may touch a load's destination SGPRs on any path from the load to the wait that drains it
(tests/test_isa_lint.py::test_no_sgpr_of_an_asm_scalar_load_is_touched_before_its_wait says why).  That test looks at the
functions named rs_score32_kernel only; this one walks the finish with the same helpers, and checks that the body was inlined
(no call) and that the kernel uses no scratch.
"""
import os
import subprocess

import pytest

from test_isa_lint import FLAGS, HIPCC, ROOT, _functions, _sregs, _walk_to_wait

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_no_sgpr_of_the_finish_kernels_scalar_loads_is_touched_before_its_wait(tmp_path):
    flags = [f for f in FLAGS if f not in ("-fno-honor-nans", "-mllvm", "-amdgpu-mfma-vgpr-form=1")]
    out = str(tmp_path / "ransac.s")
    subprocess.check_call([HIPCC, *flags, "-I" + os.path.join(ROOT, "pcreg_amd", "csrc"), "-o", out,
                           os.path.join(ROOT, "pcreg_amd", "csrc", "ransac.hip")], stderr=subprocess.DEVNULL)
    funcs = _functions(open(out).read())
    names = [n for n in funcs if "rs_bfinish_kernel" in n]
    assert len(names) == 1, names
    assert not any("rs_score32_body" in n for n in funcs), "the shared body was not inlined"
    ins = funcs[names[0]]
    assert not any(s.startswith(("scratch_", "s_swappc", "s_setpc")) for s in ins), "scratch access or a call in the finish"
    labels = {s.rstrip(":").split(":")[0]: i for i, s in enumerate(ins) if s.startswith(".LBB")}
    checked, in_asm = 0, False
    for i, s in enumerate(ins):
        if s.startswith(";;#ASMSTART"):
            in_asm = True
        elif s.startswith(";;#ASMEND"):
            in_asm = False
        elif in_asm and s.startswith("s_load_dword"):
            assert s.startswith("s_load_dwordx16"), s
            dst = _sregs(s.split(",")[0])
            assert len(dst) == 16, s
            j = next(k for k in range(i, len(ins)) if ins[k].startswith(";;#ASMEND")) + 1
            assert _walk_to_wait(ins, labels, j, dst, names[0]) > 0
            checked += 1
    assert checked >= 2, checked                     # the two alternating row sets, at least one load each
