"""The rank epilogue against its yardstick: `simrank_partial` + `combine` and `simloss_partial` + `combine` (the LSE forward) on the same
operands, timed alternately in one session with HIP events.  Shapes: the configs[2] per-rank block 4096 x 32768 x 512 and the configs[1]
head 1024 x 1024 x 512, bf16.  Appends to profiles/<prefix>_simrank_probe.log (`--log PATH` for another file)."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from x_clip_amd import _lib, ops  # noqa: E402


def log_path():
    if "--log" in sys.argv:
        return sys.argv[sys.argv.index("--log") + 1]
    prof = os.path.join(ROOT, "profiles")
    mine = sorted(glob.glob(os.path.join(prof, "r*_simrank_probe.log")))
    if mine:
        return mine[-1]
    rounds = [int(m.group(1)) for f in os.listdir(prof) for m in [re.match(r"r(\d+)_", f)] if m]
    return os.path.join(prof, f"r{max(rounds, default=0) + 1:02d}_simrank_probe.log")


def main():
    dev = torch.device("cuda:0")
    L = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    lines = [f"# tools/probe_simrank.py on {torch.cuda.get_device_name(0)}: us per (partial + combine), median of 5 rounds x 20 launches, alternating"]
    for nq, nk, d in [(4096, 32768, 512), (1024, 1024, 512)]:
        g = torch.Generator(device=dev).manual_seed(1)
        Q = torch.nn.functional.normalize(torch.randn(nq, d, device=dev, generator=g), dim=-1).bfloat16()
        K = torch.nn.functional.normalize(torch.randn(nk, d, device=dev, generator=g), dim=-1).bfloat16()
        tau = torch.tensor([2.66], device=dev)
        slots = (nk + 63) // 64
        ws = torch.empty(3 * slots * nq, dtype=torch.int32, device=dev)
        pos, lse = torch.zeros(nq, device=dev), torch.empty(nq, device=dev)
        thr, hv = torch.zeros(nq, device=dev), torch.empty(nq, device=dev)
        rank, hi = torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev)
        _lib.check(L.xclip_simrank_pos(Q.data_ptr(), K.data_ptr(), nq, nk, d, 1.0, tau.data_ptr(), 0, thr.data_ptr(), 1, st), "pos")

        def lse_fwd():
            _lib.check(L.xclip_simloss_partial(Q.data_ptr(), K.data_ptr(), nq, nk, d, 1.0, tau.data_ptr(), 0, 0, ws.data_ptr(), 0, slots,
                                               pos.data_ptr(), 1, st), "simloss_partial")
            _lib.check(L.xclip_simloss_combine(ws.data_ptr(), nq, slots, pos.data_ptr(), lse.data_ptr(), 0, 0.0, st), "simloss_combine")

        def rank_fwd():
            _lib.check(L.xclip_simrank_partial(Q.data_ptr(), K.data_ptr(), nq, nk, d, 1.0, tau.data_ptr(), 0, 0, thr.data_ptr(), ws.data_ptr(),
                                               0, slots, 1, st), "simrank_partial")
            _lib.check(L.xclip_simrank_combine(ws.data_ptr(), nq, slots, rank.data_ptr(), hv.data_ptr(), hi.data_ptr(), st), "simrank_combine")

        def timed(fn, iters=20):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) / iters * 1e3

        for fn in (lse_fwd, rank_fwd, lse_fwd, rank_fwd):
            timed(fn, 3)
        a, b = [], []
        for _ in range(5):
            a.append(timed(lse_fwd))
            b.append(timed(rank_fwd))
        a.sort()
        b.sort()
        fl = 2.0 * nq * nk * d
        lines.append(f"{nq} x {nk} x {d} bf16: LSE forward {a[2]:8.1f} us ({fl / a[2] / 1e6:6.1f} TF/s) [{a[0]:.1f} .. {a[-1]:.1f}]   "
                     f"rank {b[2]:8.1f} us ({fl / b[2] / 1e6:6.1f} TF/s) [{b[0]:.1f} .. {b[-1]:.1f}]   ratio {b[2] / a[2]:.3f}")
        lines.append(f"   (check values: recall@1 {float((rank == 0).float().mean()):.4f}, mean rank {float(rank.float().mean()):.3f}, "
                     f"max hard_val {float(hv.max()):.4f}, max |thr - forward pos| {float((thr - pos).abs().max()):.2e}: row-dot against MFMA summation order)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    path = log_path()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
