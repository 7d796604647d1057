"""The optimizer kernels' gfx950 assembly (tools/isa_scan.py, as tests/test_isa_guard.py holds the hot kernels of the step): streaming
kernels that must not spill, touch scratch or use atomics (the norm is bit-reproducible because nothing in it is atomic)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")

KERNELS = ["adamw_kernel<bf16, bf16, true>", "adamw_kernel<float, float, false>", "gradnorm_partial_kernel<bf16>",
           "adamw_kernel<bf16, float, true>", "adamw_kernel<float, bf16, false>", "gradnorm_partial_kernel<float>", "optim_prepare_kernel"]


def test_optimizer_kernels_do_not_spill_or_use_atomics(tmp_path):
    import isa_scan
    isa_scan.OUT = str(tmp_path)
    isa = isa_scan.scan(isa_scan.assemble("xclip_api.hip"))
    names = isa_scan.demangle(list(isa))
    import re
    isa = {re.sub(r"\(.*$", "", names[n]).replace("void ", "").replace("xc::", "").replace("unsigned short", "bf16"): v for n, v in isa.items()}
    for k in KERNELS:
        assert k in isa, (k, [n for n in isa if "adamw" in n or "gradnorm" in n or "optim" in n])
        s = isa[k]
        assert s["vspill"] == 0 and s["scratch"] == 0 and s["atomics"] == 0, (k, s)
