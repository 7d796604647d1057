"""The EMA update kernel's gfx950 assembly (tools/isa_scan.py, as tests/test_optim_isa.py holds adamw_kernel): one more stream of 8 floats
per thread than adamw_kernel must still not spill, touch scratch or use atomics."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")

KERNELS = ["adamw_ema_kernel<bf16, bf16, true>", "adamw_ema_kernel<float, float, false>", "adamw_ema_kernel<bf16, float, true>",
           "adamw_ema_kernel<float, bf16, false>"]


def test_ema_kernels_do_not_spill_or_use_atomics(tmp_path):
    import isa_scan
    isa_scan.OUT = str(tmp_path)
    isa = isa_scan.scan(isa_scan.assemble("xclip_api.hip"))
    names = isa_scan.demangle(list(isa))
    isa = {re.sub(r"\(.*$", "", names[n]).replace("void ", "").replace("xc::", "").replace("unsigned short", "bf16"): v for n, v in isa.items()}
    for k in KERNELS:
        assert k in isa, (k, [n for n in isa if "adamw" in n])
        s = isa[k]
        assert s["vspill"] == 0 and s["scratch"] == 0 and s["atomics"] == 0, (k, s)
