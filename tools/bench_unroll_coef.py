"""What device-resident coefficients and their gradient cost the unrolled PDE layer:
forward plus backward of 16 steps at 8 x 512^2 and 64 x 128^2, mu = 0 and 0.5, at the shipped Tb,

    by value    pis_pde_unroll_fwd + pis_pde_unroll_bwd                     (the kernels as they were)
    dev         pis_pde_unroll_fwd_dev + pis_pde_unroll_bwd_dev, g_coef NULL (coefficients from memory)
    dev + sums  the same with g_coef                                        (COEF kernels and the reduce)

and a training epoch with the fixed ``PDELayer`` against the ``LearnablePDELayer``.

    python tools/bench_unroll_coef.py                 # writes profiles/pde_unroll_coef.txt
    python tools/bench_unroll_coef.py --out FILE --rounds 15 --batch 10 --no-epoch

Per shape it times the two C calls on preallocated buffers: --batch forward + backward pairs back to
back between two HIP events, per pair. The three forms alternate inside every one of --rounds rounds
in one process and one library, so drift of the clock or of a neighbour's load falls on all of
them; the median, the minimum and the maximum over the rounds are reported. Before timing, the dev
forms' maps are compared bit for bit with the by-value form's, and the sums with
``pde.unroll_coef_vjp_np`` where the host time allows. There is no gate: the cost is reported.

The epoch: ``train_epoch`` over 4 batches of 8 synthetic images at 64^2 .. 512^2 with the Stage II
loss, ``RefinedModel`` over the fixed layer (fused AdamW) against the learnable one (fused AdamW and
the coefficients' Adam, as ``train(pde_layer_learn=...)`` runs it), 16 steps of the
reaction-diffusion preset, alternating in one process; wall time around the epoch with a device
synchronisation, median of --epochs after one warm-up each.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from physics_informed_image_segmentation_amd import _hip, pde  # noqa: E402
from bench_unroll import batched_ms, make_input  # noqa: E402

SHAPES = ((8, 512, 512), (64, 128, 128))
STEPS = 16
FORMS = ("by value", "dev", "dev + sums")


def epoch_table(say, epochs):
    from oracle import reference_torch as rt
    from physics_informed_image_segmentation_amd import AdamW, DiceBCEPDELoss, UNet
    tr = importlib.import_module("physics_informed_image_segmentation_amd.train")
    dev = torch.device("cuda")
    first = pde.PDERefine.reaction_diffusion(STEPS, 1.0, 0.5)
    say(f"\ntrain_epoch, 4 batches of 8 synthetic images, Stage II loss, metrics on: RefinedModel over the fixed layer "
        f"against LearnablePDELayer(learn = D, k, a) with its Adam ({first.steps} steps, rd preset, Tb = "
        f"{pde.unroll_temporal_block()}); wall ms per epoch, median of {epochs} (min .. max), the two alternating")
    for size in (64, 128, 256, 512):
        img, mask = rt.synthetic_batch(32, size, size, seed=5)
        batches = [(img[i:i + 8].cuda(), mask[i:i + 8].cuda()) for i in range(0, 32, 8)]
        torch.manual_seed(0)
        net = UNet(1, 1, 64).cuda()
        layer = pde.LearnablePDELayer(first, learn=("D", "k", "a")).cuda()
        models = {"fixed": pde.RefinedModel(net, first), "learnable": pde.RefinedModel(net, layer)}
        crit = DiceBCEPDELoss(pde_weight=1e-4, phase_field_weight=1e-4, diffusion_coeff=5.0).cuda()
        fused = AdamW(net.parameters(), lr=1e-5, weight_decay=1e-5)
        opts = {"fixed": fused,
                "learnable": tr._WithCoefficientAdam(fused, torch.optim.Adam(layer.parameters(), lr=1e-5))}
        times = {k: [] for k in models}
        for it in range(epochs + 1):
            for name, model in models.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.train_epoch(model, batches, crit, opts[name], dev, return_components=True)
                torch.cuda.synchronize()
                if it:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        a, b = (statistics.median(times[k]) for k in ("fixed", "learnable"))
        say(f"  {size:4d}^2: fixed {a:8.2f} ms ({min(times['fixed']):.2f} .. {max(times['fixed']):.2f})   "
            f"learnable {b:8.2f} ms ({min(times['learnable']):.2f} .. {max(times['learnable']):.2f})   "
            f"learnable / fixed = {b / a:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pde_unroll_coef.txt"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--no-epoch", action="store_true", help="skip the train_epoch table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unroll_coef: needs the GPU")
    torch.set_num_threads(1)
    lib = _hip.lib()
    st = _hip.stream_handle()
    f = ctypes.c_float
    tb = pde.unroll_temporal_block()
    lines = [f"pis_pde_unroll_fwd + _bwd against their _dev forms on {torch.cuda.get_device_name(0)}: {STEPS} steps, tile "
             f"{pde.EVOLVE_TILE[0]} x {pde.EVOLVE_TILE[1]}, shipped Tb = {tb}. Per pair = {args.batch} forward + backward C "
             f"calls on preallocated buffers between two events; the three forms alternate inside each of {args.rounds} "
             "rounds; median (min .. max) over the rounds",
             "PDE: reaction-diffusion preset, D = 1, k = 1, a = 0.5, dt = 0.5 / (4 D + k + mu), clamp on, u0 defaulted"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def check(rc):
        if rc != 0:
            raise RuntimeError(lib.pis_last_error().decode())

    for B, H, W in SHAPES:
        n = B * H * W
        u_np = make_input(B, H, W)
        g_np = (np.random.default_rng(1).random((B, H, W), dtype=np.float32) - np.float32(0.5))
        u, g_out = torch.from_numpy(u_np).cuda(), torch.from_numpy(g_np).cuda()
        out, g_u = torch.empty_like(u), torch.empty_like(u)
        ck_bytes = int(lib.pis_pde_unroll_ws(B, H, W, STEPS, tb))
        ckpt = torch.empty(max(ck_bytes, 16), dtype=torch.uint8, device="cuda")
        ws_bytes = int(lib.pis_pde_unroll_bwd_dev_ws(B, H, W))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        table = torch.empty((B, 5), dtype=torch.float64, device="cuda")
        say(f"\n{B} x {H} x {W}: map {4 * n / 1e6:.1f} MB, {ws_bytes - int(lib.pis_pde_unroll_bwd_ws(B, H, W))} bytes of slots")
        for mu in (0.0, 0.5):
            D, k, a = np.float32(1.0), np.float32(1.0), np.float32(0.5)
            _, _, _, _, muf, dt = pde._check_evolve(1, D, k, a, mu, None)
            coef = torch.tensor([D, k, a, muf, dt], dtype=torch.float32).cuda()
            fv = _hip.PIS_EVOLVE_CLAMP
            fd = fv | (_hip.PIS_EVOLVE_MU if mu else 0)

            def pair(form):
                if form == "by value":
                    check(lib.pis_pde_unroll_fwd(u.data_ptr(), 0, out.data_ptr(), ckpt.data_ptr(), ck_bytes, B, H, W, f(D),
                                                 f(k), f(a), f(muf), f(dt), STEPS, fv, tb, st))
                    check(lib.pis_pde_unroll_bwd(u.data_ptr(), 0, ckpt.data_ptr(), g_out.data_ptr(), g_u.data_ptr(), 0, B,
                                                 H, W, f(D), f(k), f(a), f(muf), f(dt), STEPS, fv, tb, ws.data_ptr(),
                                                 ws_bytes, st))
                    return
                check(lib.pis_pde_unroll_fwd_dev(u.data_ptr(), 0, out.data_ptr(), ckpt.data_ptr(), ck_bytes, B, H, W,
                                                 coef.data_ptr(), STEPS, fd, tb, st))
                check(lib.pis_pde_unroll_bwd_dev(u.data_ptr(), 0, ckpt.data_ptr(), g_out.data_ptr(), g_u.data_ptr(), 0,
                                                 table.data_ptr() if form == "dev + sums" else 0, B, H, W, coef.data_ptr(),
                                                 STEPS, fd, tb, ws.data_ptr(), ws_bytes, st))
            kept = {}
            for form in FORMS:  # warm up and check
                pair(form)
                torch.cuda.synchronize()
                kept[form] = (out.clone(), g_u.clone())
            same = all(torch.equal(kept[form][0], kept["by value"][0]) and torch.equal(kept[form][1], kept["by value"][1])
                       for form in FORMS)
            first = table.cpu().numpy()  # the warm-up's last form wrote it
            table.fill_(float("nan"))
            pair("dev + sums")
            torch.cuda.synchronize()
            again = bool((table.cpu().numpy().view(np.uint64) == first.view(np.uint64)).all())
            within = None
            if n <= 1 << 21:
                sums, abs_sums = pde.unroll_coef_vjp_np(u_np, g_np, STEPS, D, k, a, mu=mu)
                within = bool((np.abs(first - sums) <= H * W * STEPS * 2.0 ** -53 * abs_sums).all())
            times = {form: [] for form in FORMS}
            for _ in range(args.rounds):
                for form in FORMS:
                    times[form].append(batched_ms(lambda: pair(form), args.batch) * 1e3)
            say(f"  mu = {mu}: maps of the three forms equal: {same}; sums equal over two runs: {again}; sums within "
                f"H W steps 2^-53 abs_sums of unroll_coef_vjp_np: {'not compared (host time)' if within is None else within}")
            base = statistics.median(times["by value"])
            for form in FORMS:
                t = times[form]
                med = statistics.median(t)
                say(f"    {form:10s}: {med:9.1f} us ({min(t):.1f} .. {max(t):.1f})  {med / STEPS:7.2f} us per step   "
                    f"/ by value = {med / base:.3f}")
            assert same and again and within is not False
    if not args.no_epoch:
        epoch_table(say, args.epochs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"written {args.out}")


if __name__ == "__main__":
    main()
