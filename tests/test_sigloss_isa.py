"""The sigmoid-loss kernels' gfx950 assembly (tools/isa_scan.py, as tests/test_simrank_isa.py holds the rank kernels): beside the 128
accumulators the two ring-loop epilogues must not spill or touch scratch, and neither may the combine kernel."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")

KERNELS = ["sig5_loss_kernel", "sig5_grad_kernel<true>", "sig5_grad_kernel<false>", "sigloss_combine_kernel"]


def test_sigloss_kernels_do_not_spill(tmp_path):
    import isa_scan
    isa_scan.OUT = str(tmp_path)
    isa = isa_scan.scan(isa_scan.assemble("xclip_api.hip"))
    names = isa_scan.demangle(list(isa))
    isa = {re.sub(r"\(.*$", "", names[n]).replace("void ", "").replace("xc::", "").replace("unsigned short", "bf16"): v for n, v in isa.items()}
    for k in KERNELS:
        assert k in isa, (k, [n for n in isa if "sig" in n])
        s = isa[k]
        print(k, s)
        assert s["vspill"] == 0 and s["scratch"] == 0, (k, s)
