"""Distance transform and surface-distance metrics: device path (pis_edt_sq, pis_surface_distances)
against a streaming probe, one boundary_counts call and the scipy host path.

    python tools/bench_surface.py                 # writes profiles/surface_metrics.txt
    python tools/bench_surface.py --out FILE --reps 20

Every figure is the median over --reps warm calls (three calls first) of a host clock around the call
AND a device synchronise, so the kernels' time is inside the window; min and max beside it.

  * ``pis_edt_sq`` on preallocated buffers at 8 x 512^2 and 64 x 128^2: "dense" = the boundary maps of
    disc masks (what the surface metrics feed it), "corner" = one set pixel at (0, 0) (the outward
    search's worst case: every pixel crosses its whole row); for every value of pis_tune key 55 (what
    the row pass skips: nothing, 64-column blocks, 8-column steps too), alternating inside each
    repetition. The shipped value is the one with the lowest dense 8 x 512^2 time (fixed beforehand).
  * the corner case at 1 x 2048^2 against ONE ``pis_debug_stream_probe`` launch (dst = a + b) sized to
    move the transform's bytes, one uint8 read and one int32 write per pixel, best over its grid sizes.
  * ``surface_distances`` + the three scores (device) against one ``boundary_counts`` call, and against
    the same on the host path (scipy and numpy, one CPU thread).

The device tables are compared with the host's (==) before anything is timed.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physics_informed_image_segmentation_amd import _hip  # noqa: E402
from physics_informed_image_segmentation_amd import evaluate as ev  # noqa: E402

SHAPES = ((8, 512, 512), (64, 128, 128))


def discs(B, H, W, seed=42):
    """Disc masks and noisy soft copies of them as predictions."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    t = np.zeros((B, H, W), np.float32)
    for i in range(B):
        for _ in range(6):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.04, 0.12) * min(H, W)
            t[i] = np.maximum(t[i], (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r)
    noise = np.stack([ndimage.gaussian_filter(rng.standard_normal((H, W)), 3.0) for _ in range(B)])
    p = np.clip(0.8 * ndimage.gaussian_filter(t, (0, 1.5, 1.5)) + 1.5 * noise, 0, 1).astype(np.float32)
    return torch.from_numpy(p), torch.from_numpy(t)


def synced_us(fn, reps):
    """(median, min, max) in microseconds of host clock around fn() + device synchronise."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts), min(ts), max(ts)


def alternating_us(fns, reps):
    """synced_us for several callables, taking turns inside each repetition."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for acc, fn in zip(ts, fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e6)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


PRUNE = ((0, "plain outward search"), (1, "64-column blocks skipped"), (3, "blocks and 8-column steps skipped"))


def fmt(t):
    return f"{t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_metrics.txt"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface: needs the GPU")
    torch.set_num_threads(1)
    lib = _hip.lib()
    st = _hip.stream_handle()
    lines = [f"distance transform and surface metrics on {torch.cuda.get_device_name(0)}: median of {args.reps} warm "
             f"calls, host clock around the call and a device synchronise"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def check(rc):
        if rc != 0:
            raise RuntimeError(lib.pis_last_error().decode())

    def edt_timer(sets):
        """(timings of pis_edt_sq on preallocated buffers per value of key 55, the shipped value's output)"""
        N, H, W = sets.shape
        nbytes = lib.pis_edt_ws(N, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        d2 = torch.empty((N, H, W), dtype=torch.int32, device="cuda")

        def run(v):
            prev = lib.pis_tune(_hip.PIS_TUNE_EDT_PRUNE, v)
            try:
                check(lib.pis_edt_sq(sets.data_ptr(), N, H, W, d2.data_ptr(), ws.data_ptr(), nbytes, st))
            finally:
                lib.pis_tune(_hip.PIS_TUNE_EDT_PRUNE, prev)
        ts = alternating_us([lambda v=v: run(v) for v, _ in PRUNE], args.reps)
        run(lib.pis_tune(_hip.PIS_TUNE_EDT_PRUNE, -1))
        return ts, d2

    def corner(N, H, W):
        m = torch.zeros((N, H, W), dtype=torch.uint8)
        m[:, 0, 0] = 1
        return m

    for B, H, W in SHAPES:
        say(f"\n{B} x {H} x {W}")
        p, t = discs(B, H, W)
        pc, tc = p.cuda(), t.cuda()
        bnd = ev.extract_boundaries_device(tc)
        for name, sets in (("dense (disc boundaries)", bnd), ("corner (one set pixel)", corner(B, H, W).cuda())):
            ts, d2 = edt_timer(sets)
            ok = np.array_equal(d2.cpu().numpy(), ev.distance_transform_sq_np(sets.cpu().numpy()))
            say(f"  pis_edt_sq {name}: matches host: {ok}")
            for (v, what), tm in zip(PRUNE, ts):
                say(f"    key 55 = {v} ({what}): {fmt(tm)}, {5 * B * H * W / tm[0] / 1e6:.3f} TB/s of the 5 B per pixel")
            assert ok

        def device_path():
            pair = ev.surface_distances(pc, tc)
            return torch.stack([ev.compute_hausdorff_percentile_batch(pair), ev.compute_assd_batch(pair),
                                ev.compute_surface_dice_batch(pair)])

        def host_path():
            pair = ev.surface_distances(p, t)
            return torch.stack([ev.compute_hausdorff_percentile_batch(pair), ev.compute_assd_batch(pair),
                                ev.compute_surface_dice_batch(pair)])
        dev_pair, host_pair = ev.surface_distances(pc, tc), ev.surface_distances(p, t)
        ok = torch.equal(dev_pair[0].cpu(), host_pair[0]) and torch.equal(dev_pair[1].cpu(), host_pair[1])
        t_dev = synced_us(device_path, args.reps)
        t_pair = synced_us(lambda: ev.surface_distances(pc, tc), args.reps)
        t_cnt = synced_us(lambda: ev.boundary_counts(pc, tc, 0.5, 2), args.reps)
        t0 = time.perf_counter()
        host_path()
        host_us = (time.perf_counter() - t0) * 1e6
        say(f"  surface_distances + HD95 + ASSD + surface Dice: {fmt(t_dev)}; surface_distances alone: {fmt(t_pair)}; "
            f"one boundary_counts call: {fmt(t_cnt)} ({t_dev[0] / t_cnt[0]:.2f} x); host path (scipy, one thread, one "
            f"run): {host_us / 1e3:.1f} ms ({host_us / t_dev[0]:.0f} x); tables match host: {ok}")
        assert ok

    N, H, W = 1, 2048, 2048
    say(f"\n{N} x {H} x {W}, corner (one set pixel)")
    sets = corner(N, H, W).cuda()
    ts, d2 = edt_timer(sets)
    tm = ts[[v for v, _ in PRUNE].index(lib.pis_tune(_hip.PIS_TUNE_EDT_PRUNE, -1))]
    yy, xx = np.mgrid[:H, :W]
    ok = np.array_equal(d2[0].cpu().numpy(), yy * yy + xx * xx)
    n = (5 * N * H * W // 12) // 4 * 4          # floats: 12 B each through dst = a + b
    a, b, dst = (torch.zeros(n, device="cuda") for _ in range(3))
    probe, grid = min((synced_us(lambda g=g: check(lib.pis_debug_stream_probe(
        a.data_ptr(), b.data_ptr(), dst.data_ptr(), n, 0, g, st)), args.reps), g) for g in (256, 512, 1024, 2048, 4096))
    for (v, what), t in zip(PRUNE, ts):
        say(f"    key 55 = {v} ({what}): {fmt(t)}")
    say(f"  pis_edt_sq as shipped: {fmt(tm)}; one stream probe launch over the same {12 * n / 1e6:.1f} MB: {fmt(probe)} (grid "
        f"{grid}); ratio {tm[0] / probe[0]:.2f} x; matches y^2 + x^2: {ok}")
    assert ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written {args.out}")


if __name__ == "__main__":
    main()
