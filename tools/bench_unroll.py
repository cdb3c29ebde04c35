"""The unrolled PDE layer (pis_pde_unroll_fwd + pis_pde_unroll_bwd): forward plus backward for every
temporal block Tb side by side, against eager-torch autograd of the same steps and one bandwidth
probe, at 8 x 512^2 and 64 x 128^2 for 8 and 16 steps; and a training epoch with the layer on
against off.

    python tools/bench_unroll.py                 # writes profiles/pde_unroll.txt
    python tools/bench_unroll.py --out FILE --rounds 15 --batch 10 --no-epoch

Per shape and step count it times the two C calls on preallocated buffers (no allocation, no Python
around them but ctypes): --batch forward + backward pairs back to back between two HIP events, per
pair. The values of Tb (1, 2, 4) alternate inside every one of --rounds rounds in one process and
one library, so drift of the clock or of a neighbour's load falls on all of them; the median, the
minimum and the maximum over the rounds are reported. Every Tb's gradient is compared bit for bit
with Tb = 1's first, and with ``pde.unroll_vjp_np`` where the host time allows.

Yardsticks at the same shape: ``pde.unroll`` + ``backward`` through autograd (the same two calls
plus torch's allocations and graph); the steps restated in eager torch and differentiated by
autograd; ONE ``pis_debug_stream_probe`` launch (dst = a + b, 12 B per element) sized to move the
bytes the two chains read and write at that Tb (forward: a map read and a map written per launch,
plus u0 with mu; backward: the state and the gradient read, the gradient written, plus u0 and the
running sum both ways with mu), best over its grid sizes.

The rule for the shipped Tb, fixed before measuring: the lowest forward-plus-backward time of 16
steps at 8 x 512^2, mu = 0, clamp on.

The epoch: ``train_epoch`` over 4 batches of 8 synthetic images at 64^2 .. 512^2 with the Stage II
loss, the plain U-Net against ``RefinedModel`` (16 steps of the reaction-diffusion preset),
alternating in one process; wall time around the epoch with a device synchronisation, median of
--epochs after one warm-up each.
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physics_informed_image_segmentation_amd import _hip, pde  # noqa: E402

SHAPES = ((8, 512, 512), (64, 128, 128))
STEPS = (8, 16)
RULE = (8, 512, 512, 16, 0.0)


def make_input(B, H, W):
    """A smooth map in (0, 1): a sigmoid of box-filtered noise."""
    g = torch.Generator().manual_seed(42)
    f = torch.randn((B, 1, H, W), generator=g)
    for _ in range(3):
        f = Fn.avg_pool2d(Fn.pad(f, (3, 3, 3, 3), mode="reflect"), 7, stride=1)
    return torch.sigmoid(12.0 * f / f.std())[:, 0].contiguous().numpy().astype(np.float32)


def unroll_torch(u, steps, D, k, a, mu, dt, clamp=True):
    """evolve_np in eager torch, differentiable by autograd."""
    c, z = u, u
    for _ in range(steps):
        p = Fn.pad(c[:, None], (1, 1, 1, 1), mode="reflect")[:, 0]
        up, dn, lf, rt = p[:, :-2, 1:-1], p[:, 2:, 1:-1], p[:, 1:-1, :-2], p[:, 1:-1, 2:]
        lap = ((up + dn) + (lf + rt)) - 4.0 * c
        t = D * lap + k * ((c * (1.0 - c)) * (c - a))
        if mu != 0:
            t = t + mu * (z - c)
        c = c + dt * t
        if clamp:
            c = c.clamp(0.0, 1.0)
    return c


def batched_ms(fn, batch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(batch):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / batch


def epoch_table(say, epochs):
    from oracle import reference_torch as rt
    from physics_informed_image_segmentation_amd import AdamW, DiceBCEPDELoss, UNet
    tr = importlib.import_module("physics_informed_image_segmentation_amd.train")
    dev = torch.device("cuda")
    layer = pde.PDERefine.reaction_diffusion(16, 1.0, 0.5)
    say(f"\ntrain_epoch, 4 batches of 8 synthetic images, Stage II loss, metrics on: plain U-Net against RefinedModel "
        f"({layer.steps} steps, rd preset, Tb = {pde.unroll_temporal_block()}); wall ms per epoch, median of {epochs} "
        "(min .. max), the two alternating")
    for size in (64, 128, 256, 512):
        img, mask = rt.synthetic_batch(32, size, size, seed=5)
        batches = [(img[i:i + 8].cuda(), mask[i:i + 8].cuda()) for i in range(0, 32, 8)]
        torch.manual_seed(0)
        net = UNet(1, 1, 64).cuda()
        models = {"off": net, "on": pde.RefinedModel(net, layer)}
        crit = DiceBCEPDELoss(pde_weight=1e-4, phase_field_weight=1e-4, diffusion_coeff=5.0).cuda()
        opt = AdamW(net.parameters(), lr=1e-5, weight_decay=1e-5)
        times = {k: [] for k in models}
        for it in range(epochs + 1):
            for name, model in models.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.train_epoch(model, batches, crit, opt, dev, return_components=True)
                torch.cuda.synchronize()
                if it:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        off, on = (statistics.median(times[k]) for k in ("off", "on"))
        say(f"  {size:4d}^2: off {off:8.2f} ms ({min(times['off']):.2f} .. {max(times['off']):.2f})   "
            f"on {on:8.2f} ms ({min(times['on']):.2f} .. {max(times['on']):.2f})   on / off = {on / off:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pde_unroll.txt"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--no-epoch", action="store_true", help="skip the train_epoch table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unroll: needs the GPU")
    torch.set_num_threads(1)
    lib = _hip.lib()
    st = _hip.stream_handle()
    f = ctypes.c_float
    shipped = pde.unroll_temporal_block()
    lines = [f"pis_pde_unroll_fwd + pis_pde_unroll_bwd on {torch.cuda.get_device_name(0)}: tile {pde.EVOLVE_TILE[0]} x "
             f"{pde.EVOLVE_TILE[1]}, shipped Tb = {shipped}. Per pair = {args.batch} forward + backward C calls on "
             f"preallocated buffers between two events; Tb alternates inside each of {args.rounds} rounds; median "
             "(min .. max) over the rounds",
             "PDE: reaction-diffusion preset, D = 1, k = 1, a = 0.5, dt = 0.5 / (4 D + k + mu), clamp on, u0 defaulted; "
             "mu = 0 and mu = 0.5 (u0 plane and running sum staged)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def check(rc):
        if rc != 0:
            raise RuntimeError(lib.pis_last_error().decode())

    totals = {}
    for B, H, W in SHAPES:
        n = B * H * W
        u_np = make_input(B, H, W)
        g_np = (np.random.default_rng(1).random((B, H, W), dtype=np.float32) - np.float32(0.5))
        u, g_out = torch.from_numpy(u_np).cuda(), torch.from_numpy(g_np).cuda()
        out, g_u = torch.empty_like(u), torch.empty_like(u)
        ck_bytes = int(lib.pis_pde_unroll_ws(B, H, W, max(STEPS), 1))
        ckpt = torch.empty(max(ck_bytes, 16), dtype=torch.uint8, device="cuda")
        ws_bytes = int(lib.pis_pde_unroll_bwd_ws(B, H, W))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        partial = torch.empty(16384, device="cuda")
        say(f"\n{B} x {H} x {W}: map {4 * n / 1e6:.1f} MB")
        for mu in (0.0, 0.5):
            D, k, a = np.float32(1.0), np.float32(1.0), np.float32(0.5)
            _, _, _, _, muf, dt = pde._check_evolve(1, D, k, a, mu, None)
            for steps in STEPS:
                if mu != 0.0 and steps != 16:
                    continue
                flags = _hip.PIS_EVOLVE_CLAMP

                def pair(tb):
                    check(lib.pis_pde_unroll_fwd(u.data_ptr(), 0, out.data_ptr(), ckpt.data_ptr(), ck_bytes, B, H, W, f(D),
                                                 f(k), f(a), f(muf), f(dt), steps, flags, tb, st))
                    check(lib.pis_pde_unroll_bwd(u.data_ptr(), 0, ckpt.data_ptr(), g_out.data_ptr(), g_u.data_ptr(), 0, B,
                                                 H, W, f(D), f(k), f(a), f(muf), f(dt), steps, flags, tb, ws.data_ptr(),
                                                 ws_bytes, st))
                grads = {}
                for tb in pde.UNROLL_TB_VALUES:  # warm up and check
                    pair(tb)
                    torch.cuda.synchronize()
                    grads[tb] = (out.clone(), g_u.clone())
                same_tb = all(torch.equal(grads[tb][0], grads[1][0]) and torch.equal(grads[tb][1], grads[1][1])
                              for tb in grads)
                same_np = None
                if B * H * W <= 1 << 21:
                    want, _ = pde.unroll_vjp_np(u_np, g_np, steps, D, k, a, mu=mu)
                    same_np = bool((grads[1][1].cpu().numpy().view(np.uint32) == want.view(np.uint32)).all())

                def eager():
                    leaf = u.detach().requires_grad_()
                    unroll_torch(leaf, steps, float(D), float(k), float(a), float(muf), float(dt)).backward(g_out)
                    return leaf.grad

                def autograd():
                    leaf = u.detach().requires_grad_()
                    pde.unroll(leaf, steps=steps, D=D, k=k, a=a, mu=mu).backward(g_out)
                    return leaf.grad
                ge = eager()
                rel = float((ge - grads[1][1]).abs().max() / grads[1][1].abs().max())
                same_auto = torch.equal(autograd(), grads[shipped][1])
                times = {tb: [] for tb in pde.UNROLL_TB_VALUES}
                for _ in range(args.rounds):
                    for tb in pde.UNROLL_TB_VALUES:
                        times[tb].append(batched_ms(lambda: pair(tb), args.batch) * 1e3)
                few = max(3, args.rounds // 3)
                eager_t = [batched_ms(eager, 2) * 1e3 for _ in range(few)]
                auto_t = [batched_ms(autograd, args.batch) * 1e3 for _ in range(few)]
                say(f"  steps = {steps}, mu = {mu}: all Tb equal: {same_tb}; equals unroll_vjp_np: "
                    f"{'not compared (host time)' if same_np is None else same_np}; pde.unroll + backward equal: {same_auto}; "
                    f"eager autograd max-norm relative difference {rel:.2e}")
                for tb in pde.UNROLL_TB_VALUES:
                    launches = -(-steps // tb)
                    maps = launches * (5 + (4 if mu else 0))      # fwd 2 (+1), bwd 3 (+3: u0, the sum in and out)
                    nf = -(-(maps * 4 * n) // 48) * 4
                    pa, pb, pd = (torch.empty(nf, device="cuda").uniform_() for _ in range(3))
                    probe_us = min(statistics.median(
                        batched_ms(lambda gr=gr: check(lib.pis_debug_stream_probe(pa.data_ptr(), pb.data_ptr(), pd.data_ptr(),
                                                                                  nf, partial.data_ptr(), gr, st)), 5)
                        for _ in range(5)) * 1e3 for gr in (1024, 2048, 4096, 8192))
                    del pa, pb, pd
                    t = times[tb]
                    med = statistics.median(t)
                    say(f"    Tb = {tb}: {med:9.1f} us ({min(t):.1f} .. {max(t):.1f})  {med / steps:7.2f} us per step, "
                        f"{2 * launches} launches; probe of their {maps} map passes {probe_us:.1f} us: {med / probe_us:5.2f} x")
                    totals[(B, H, W, steps, mu, tb)] = med
                for name, ts in (("pde.unroll + backward (autograd, allocations)", auto_t), ("eager torch autograd", eager_t)):
                    med = statistics.median(ts)
                    say(f"    {name}: {med:9.1f} us ({min(ts):.1f} .. {max(ts):.1f})  {med / steps:7.2f} us per step")
                assert same_tb and same_auto and same_np is not False and rel < 1e-4
    best = min(pde.UNROLL_TB_VALUES, key=lambda tb: totals[RULE + (tb,)])
    say(f"\nlowest forward-plus-backward time of 16 steps at 8 x 512^2 (mu = 0, clamp on): Tb = {best}; shipped Tb = {shipped}")
    if not args.no_epoch:
        epoch_table(say, args.epochs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written {args.out}")


if __name__ == "__main__":
    main()
