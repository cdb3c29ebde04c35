"""Boundary F1 / Hausdorff: device path (pis_boundary_metrics) against the host path, at 8 x 512^2.

    python tools/bench_boundary.py --part a    # device time per call: disc masks, noisy blobs
    python tools/bench_boundary.py --part b    # host path on the same inputs
    python tools/bench_boundary.py --part c    # train_epoch images/s, boundary_backend host / device

(a) times ``evaluate.boundary_counts`` (the nine launches plus the workspace allocation from the
caching allocator) with HIP events, median of --reps warm calls, and checks the counters against
the host path once. (b) times ``compute_boundary_f1_batch(backend="host")`` and the per-image
``compute_hausdorff_distance`` of the host path with a host clock, one image at a time as
``evaluate_model`` runs them; the host scorer of the step loop spreads the F1 part over up to 8
threads. (c) runs ``train_epoch`` over 64 synthetic disc images (DeviceDiscLoader, batch 8, the
C2 model and loss) with the two backends alternating in one process, after one warm-up epoch
each; ``train_epoch`` ends in its host synchronisation, so a host clock around it is the epoch
time. Each part is one process: run each under its own time limit.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physics_informed_image_segmentation_amd import evaluate as ev  # noqa: E402

B, H, W = 8, 512, 512


def disc_inputs():
    """Masks of the synthetic generator; predictions = the neighbouring sample's mask (two clean
    disc sets that overlap partly), as probabilities 0.05 / 0.95."""
    from physics_informed_image_segmentation_amd.dataset import SyntheticDiscDataset
    ds = SyntheticDiscDataset(B + 1, (H, W), seed=42)
    m = torch.stack([ds[i][1][0] for i in range(B + 1)])
    return (m[1:] * 0.9 + 0.05).contiguous(), m[:B].contiguous()


def blob_inputs(seed=11, sigma=3.0):
    """Seeded Gaussian-filtered noise cut at its middle: the ragged masks an untrained network
    produces (tests/test_boundary_gpu.py::_blobs at full size)."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)

    def field():
        f = np.stack([ndimage.gaussian_filter(rng.standard_normal((H, W)), sigma) for _ in range(B)])
        return (f - f.min()) / (f.max() - f.min())
    return torch.from_numpy(field().astype(np.float32)), torch.from_numpy((field() > 0.5).astype(np.float32))


INPUTS = (("discs", disc_inputs), ("blobs", blob_inputs))


def part_a(args):
    for name, make in INPUTS:
        p, t = make()
        pc, tc = p.cuda(), t.cuda()
        counts = ev.boundary_counts(pc, tc, 0.5, 2)
        for _ in range(5):
            ev.boundary_counts(pc, tc, 0.5, 2)
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ev.boundary_counts(pc, tc, 0.5, 2)
            e1.record()
            ms.append((e0, e1))
        torch.cuda.synchronize()
        t_ms = sorted(a.elapsed_time(b) for a, b in ms)
        c = counts.cpu().numpy()
        # exactness at the timed size, first two samples (the host path is the slow side)
        f1_dev = ev.compute_boundary_f1_batch(pc[:2, None], tc[:2, None]).cpu()
        f1_host = ev.compute_boundary_f1_batch(p[:2, None], t[:2, None], backend="host")
        hd_dev = ev.compute_hausdorff_distance_batch(pc[:2], tc[:2]).cpu().numpy()
        hd_host = [ev.compute_hausdorff_distance(p[i:i + 1, None], t[i:i + 1, None]) for i in range(2)]
        ok = bool((f1_dev - f1_host).abs().max() <= 1e-6 and all(hd_dev[i] == hd_host[i] for i in range(2)))
        print(f"(a) {name}: pis_boundary_metrics {B}x{H}x{W}: median {t_ms[len(t_ms) // 2]:.3f} ms per call "
              f"(min {t_ms[0]:.3f}, max {t_ms[-1]:.3f}, {args.reps} calls), boundary pixels per image "
              f"pred {c[:, 0].mean():.0f} target {c[:, 1].mean():.0f}, matches host: {ok}", flush=True)
        assert ok


def part_b(args):
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    for name, make in INPUTS:
        p, t = make()
        p4, t4 = p[:, None], t[:, None]
        ev.compute_boundary_f1_batch(p4[:1], t4[:1], backend="host")
        t0 = time.perf_counter()
        ev.compute_boundary_f1_batch(p4, t4, backend="host")
        f1_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for i in range(B):
            ev.compute_hausdorff_distance(p4[i:i + 1], t4[i:i + 1], backend="host")
        hd_ms = (time.perf_counter() - t0) * 1e3
        print(f"(b) {name}: host path {B}x{H}x{W}: boundary F1 {f1_ms:.1f} ms per batch ({f1_ms / B:.1f} ms per image), "
              f"Hausdorff {hd_ms:.1f} ms per batch ({hd_ms / B:.1f} ms per image), one thread; "
              f"{len(os.sched_getaffinity(0))} CPUs visible", flush=True)


def part_c(args):
    import importlib
    from physics_informed_image_segmentation_amd import AdamW, DiceBCEPDELoss, UNet
    from physics_informed_image_segmentation_amd.dataset import DeviceDiscLoader
    tr = importlib.import_module("physics_informed_image_segmentation_amd.train")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = UNet(1, 1, 64).to(dev)
    crit = DiceBCEPDELoss(pde_weight=1e-4, phase_field_weight=1e-4, diffusion_coeff=5.0, reaction_threshold=0.5,
                          epsilon=0.05)
    opt = AdamW(net.parameters(), lr=1e-4, weight_decay=1e-5)
    n = 64
    loader = DeviceDiscLoader(n, B, (H, W), seed=42, shuffle=False, device=dev)

    def epoch(backend):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.train_epoch(net, loader, crit, opt, dev, boundary_backend=backend)
        return n / (time.perf_counter() - t0), res["boundary_f1_score"]

    for be in ("host", "device"):
        epoch(be)
    rates = {"host": [], "device": [], "off": []}
    for _ in range(args.rounds):
        for be in ("host", "device"):
            r, f1 = epoch(be)
            rates[be].append(r)
            print(f"    {be}: {r:.1f} images/s (boundary_f1_score {f1:.4f})", flush=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.train_epoch(net, loader, crit, opt, dev, boundary_metrics=False)
        rates["off"].append(n / (time.perf_counter() - t0))
    for be in ("host", "device", "off"):
        r = sorted(rates[be])
        print(f"(c) train_epoch {n} images {B}x{H}x{W}, boundary {be}: median {r[len(r) // 2]:.1f} images/s "
              f"(min {r[0]:.1f}, max {r[-1]:.1f}, {len(r)} epochs, alternating)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("a", "b", "c"), required=True)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.part != "b" and not torch.cuda.is_available():
        raise SystemExit("bench_boundary: parts a and c need the GPU")
    {"a": part_a, "b": part_b, "c": part_c}[args.part](args)


if __name__ == "__main__":
    main()
