"""The sigmoid-loss kernels against their yardsticks, the InfoNCE kernels on the same operands, timed alternately in one session with HIP
events: `sigloss_partial` + `combine` against `simloss_partial` + `combine` (the LSE forward), and `sigloss_grad` against `simloss_grad`.
Shapes: the configs[2] per-rank block 4096 x 32768 x 512 and the configs[1] head 1024 x 1024 x 512, bf16; medians of 5 rounds x 20 launches.
Appends to profiles/<prefix>_sigloss_probe.log (`--log PATH` for another file)."""
import glob
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from x_clip_amd import _lib  # noqa: E402


def log_path():
    if "--log" in sys.argv:
        return sys.argv[sys.argv.index("--log") + 1]
    prof = os.path.join(ROOT, "profiles")
    mine = sorted(glob.glob(os.path.join(prof, "r*_sigloss_probe.log")))
    if mine:
        return mine[-1]
    rounds = [int(m.group(1)) for f in os.listdir(prof) for m in [re.match(r"r(\d+)_", f)] if m]
    return os.path.join(prof, f"r{max(rounds, default=0) + 1:02d}_sigloss_probe.log")


def main():
    dev = torch.device("cuda:0")
    L = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    lines = [f"# tools/probe_sigloss.py on {torch.cuda.get_device_name(0)}: us per call, median of 5 rounds x 20 launches, alternating"]
    for nq, nk, d in [(4096, 32768, 512), (1024, 1024, 512)]:
        g = torch.Generator(device=dev).manual_seed(1)
        Q = torch.nn.functional.normalize(torch.randn(nq, d, device=dev, generator=g), dim=-1).bfloat16()
        K = torch.nn.functional.normalize(torch.randn(nk, d, device=dev, generator=g), dim=-1).bfloat16()
        tau = torch.tensor([math.log(10.0)], device=dev)
        beta = torch.tensor([-10.0], device=dev)
        gmul = torch.ones(1, device=dev)
        slots = (nk + 63) // 64
        ws = torch.empty(2 * slots * nq, dtype=torch.float32, device=dev)
        pos, lse, rowloss = torch.zeros(nq, device=dev), torch.empty(nq, device=dev), torch.empty(nq, device=dev)
        loss = torch.zeros(1, device=dev)
        G = torch.empty(nq, nk, dtype=torch.bfloat16, device=dev)
        dtau, dbeta = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        B = float(nk)

        def lse_fwd():
            _lib.check(L.xclip_simloss_partial(Q.data_ptr(), K.data_ptr(), nq, nk, d, 1.0, tau.data_ptr(), 0, 0, ws.data_ptr(), 0, slots,
                                               pos.data_ptr(), 1, st), "simloss_partial")
            _lib.check(L.xclip_simloss_combine(ws.data_ptr(), nq, slots, pos.data_ptr(), lse.data_ptr(), loss.data_ptr(), 0.5 / B, st), "simloss_combine")

        def sig_fwd():
            _lib.check(L.xclip_sigloss_partial(Q.data_ptr(), K.data_ptr(), nq, nk, d, 1.0, tau.data_ptr(), beta.data_ptr(), 0, ws.data_ptr(), 0,
                                               slots, 1, st), "sigloss_partial")
            _lib.check(L.xclip_sigloss_combine(ws.data_ptr(), nq, slots, rowloss.data_ptr(), loss.data_ptr(), 1.0 / B, st), "sigloss_combine")

        def lse_grad():
            _lib.check(L.xclip_simloss_grad(Q.data_ptr(), K.data_ptr(), nq, nk, d, 1.0, tau.data_ptr(), 0, 0, 0.5 / B, 0.5 / B, 1.0 / B,
                                            gmul.data_ptr(), 1, lse.data_ptr(), lse_k.data_ptr(), G.data_ptr(), nk, dtau.data_ptr(), 1, st),
                       "simloss_grad")

        def sig_grad():
            _lib.check(L.xclip_sigloss_grad(Q.data_ptr(), K.data_ptr(), nq, nk, d, 1.0, tau.data_ptr(), beta.data_ptr(), 0, 1.0 / B,
                                            gmul.data_ptr(), 1, G.data_ptr(), nk, dtau.data_ptr(), dbeta.data_ptr(), 1, st), "sigloss_grad")

        def timed(fn, iters=20):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) / iters * 1e3

        # the column log-sum-exps the InfoNCE G needs: the transposed forward (K's rows against Q), as the loss's second direction forms them
        ws_k = torch.empty(2 * ((nq + 63) // 64) * nk, dtype=torch.float32, device=dev)
        pos_k, lse_k = torch.zeros(nk, device=dev), torch.empty(nk, device=dev)
        _lib.check(L.xclip_simloss_partial(K.data_ptr(), Q.data_ptr(), nk, nq, d, 1.0, tau.data_ptr(), 0, 0, ws_k.data_ptr(), 0, (nq + 63) // 64,
                                           pos_k.data_ptr(), 1, st), "simloss_partial (columns)")
        _lib.check(L.xclip_simloss_combine(ws_k.data_ptr(), nk, (nq + 63) // 64, pos_k.data_ptr(), lse_k.data_ptr(), 0, 0.0, st), "simloss_combine (columns)")
        lse_fwd()
        fl = 2.0 * nq * nk * d
        for name, base, mine in (("forward (partial + combine)", lse_fwd, sig_fwd), ("G", lse_grad, sig_grad)):
            for fn in (base, mine, base, mine):
                timed(fn, 3)
            a, b = [], []
            for _ in range(5):
                a.append(timed(base))
                b.append(timed(mine))
            a.sort()
            b.sort()
            lines.append(f"{nq} x {nk} x {d} bf16 {name}: InfoNCE {a[2]:8.1f} us ({fl / a[2] / 1e6:6.1f} TF/s) [{a[0]:.1f} .. {a[-1]:.1f}]   "
                         f"sigmoid {b[2]:8.1f} us ({fl / b[2] / 1e6:6.1f} TF/s) [{b[0]:.1f} .. {b[-1]:.1f}]   ratio {b[2] / a[2]:.3f}")
        lines.append(f"   (check values: mean rowloss {float(rowloss.mean()):.6e}, max |G| {float(G.float().abs().max()):.3e})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    path = log_path()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
