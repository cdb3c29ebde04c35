"""Tiled, test-time-augmented prediction: the two launches around the forwards, the end-to-end rate and
the eager-torch alternative, at 8 x 512^2 (S = 8) and one 2048^2 image, tile 512, overlap 64, without
test-time augmentation and with all eight symmetries.

    python tools/bench_predict.py                 # writes profiles/predict.txt
    python tools/bench_predict.py --out FILE --reps 30 --e2e-reps 5

Per configuration:

(a) ``pis_tile_gather`` (one chunk of --batch-tiles jobs) and ``pis_tile_blend`` (all jobs) per launch,
    HIP events, median of --reps: cold (a 1 GiB read between launches, bench.py's protocol) and warm
    (back to back). Beside each ONE ``pis_debug_stream_probe`` launch (dst = a + b, 12 B per element)
    over as many floats as make its bytes equal the kernel's algorithmic bytes — gather: the chunk's
    elements read once and written once; blend: every tile output read once, prob (4 B) and mask (1 B)
    written per pixel — same protocol, best over the probe's grid sizes. The convention of
    profiles/device_cache.txt.
(b) end to end: ``Predictor.predict_batch`` per call (events around the call, then one synchronise;
    median of --e2e-reps), beside the forwards alone: the same number of ``model(tiles)`` calls on a
    resident chunk, nothing else. Their difference is what the gathers, the copies into the tile-output
    buffer and the blend cost when they run between forwards.
(c) the alternative the two kernels replace, in eager torch with the same tiling: reflect-index rows
    and columns, flip / transpose per job, forward, and a weighted ``+=`` per job into an accumulator,
    one division at the end. Timed end to end like (b), and its data movement alone (everything but
    the forwards, on given tile outputs) beside the kernels' data movement alone (every gather of the
    image and the blend). The eager result is compared with the kernels' (max abs difference printed;
    it orders its sums the same way but fuses nothing, so it is expected to be 0).

There is no time gate on this path: the file records what was measured, nothing more.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physics_informed_image_segmentation_amd import _hip  # noqa: E402
from physics_informed_image_segmentation_amd import predict as pr  # noqa: E402
from physics_informed_image_segmentation_amd.dataset import apply_symmetry  # noqa: E402

CONFIGS = (("8 x 512^2", 8, 512, 512), ("1 x 2048^2", 1, 2048, 2048))
TTAS = (None, "d4")
PROBE_GRIDS = (256, 512, 1024, 2048, 4096, 8192)


def event_ms(fn, reps, flush=None, sink=None):
    evs = []
    for _ in range(reps + 3):
        if flush is not None:
            torch.sum(flush, dim=0, out=sink)  # a READ: evicts with clean lines (no write-back tail)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in evs[3:])


def invert_symmetry(t, q):
    if q & 4:
        t = t.transpose(-1, -2)
    if q & 2:
        t = t.flip(-2)
    if q & 1:
        t = t.flip(-1)
    return t


class EagerTiling:
    """The same tiling in eager torch ops (any device): what the two kernels replace."""

    def __init__(self, plan, S, device, threshold=0.5):
        self.plan, self.S, self.threshold = plan, S, threshold
        self.rows = [torch.from_numpy(pr.reflect_index(y0 + np.arange(plan.th), plan.H)).to(device) for y0 in plan.oy]
        self.cols = [torch.from_numpy(pr.reflect_index(x0 + np.arange(plan.tw), plan.W)).to(device) for x0 in plan.ox]
        wy = torch.from_numpy(pr.ramp_weights(plan.th, plan.ov)).to(device)
        wx = torch.from_numpy(pr.ramp_weights(plan.tw, plan.ov)).to(device)
        self.w = (wy[:, None] * wx[None, :]).to(torch.float32)

    def job(self, j):
        p = self.plan
        t, qi = divmod(j, p.Ns)
        t, kx = divmod(t, p.Kx)
        s, ky = divmod(t, p.Ky)
        return s, ky, kx, p.codes[qi]

    def gather(self, x, first, n):
        """x (S, H, W) -> (n, 1, th, tw)."""
        tiles = []
        for j in range(first, first + n):
            s, ky, kx, q = self.job(j)
            T = x[s].index_select(0, self.rows[ky]).index_select(1, self.cols[kx])
            tiles.append(apply_symmetry(T, q))
        return torch.stack(tiles)[:, None]

    def blend(self, u):
        p = self.plan
        acc = torch.zeros((self.S, p.H, p.W), dtype=torch.float32, device=u.device)
        wsum = torch.zeros_like(acc)
        for j in range(p.jobs(self.S)):
            s, ky, kx, q = self.job(j)
            y0, x0 = p.oy[ky], p.ox[kx]
            hh, ww = min(p.th, p.H - y0), min(p.tw, p.W - x0)
            w = self.w[:hh, :ww]
            acc[s, y0:y0 + hh, x0:x0 + ww] += w * invert_symmetry(u[j, 0], q)[:hh, :ww]
            if q == p.codes[0]:
                wsum[s, y0:y0 + hh, x0:x0 + ww] += w * p.Ns
        prob = acc / wsum
        return prob, (prob > self.threshold).to(torch.uint8)

    def predict(self, model, x, batch_tiles):
        J = self.plan.jobs(self.S)
        n, starts = pr.chunk_starts(J, batch_tiles)
        u = torch.empty((J, 1, self.plan.th, self.plan.tw), dtype=torch.float32, device=x.device)
        done = 0
        for first in starts:
            out = model(self.gather(x, first, n))
            u[done:first + n] = out[done - first:]
            done = first + n
        return self.blend(u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--batch-tiles", type=int, default=8)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict: needs the GPU")
    from physics_informed_image_segmentation_amd import UNet
    lib = _hip.lib()
    st = _hip.stream_handle()
    dev = torch.device("cuda")
    torch.manual_seed(42)
    model = UNet(1, 1, 64).to(dev).eval()
    flush = torch.ones(256 << 20, device=dev)  # 1 GiB
    sink = torch.empty((), device=dev)
    lines = [f"tools/bench_predict.py --reps {args.reps} --e2e-reps {args.e2e_reps} --batch-tiles {args.batch_tiles} "
             f"--tile {args.tile} --overlap {args.overlap}   [{torch.cuda.get_device_name(0)}, torch {torch.__version__}]",
             "no time gate on this path: measurements only"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def check(rc):
        if rc != 0:
            raise RuntimeError(lib.pis_last_error().decode())

    def probe_ms(nbytes, fl):
        nf = -(-nbytes // 48) * 4  # floats per probe array: 12 B per element, n % 4 == 0
        a, b, dst = (torch.ones(nf, device=dev) for _ in range(3))
        return min((event_ms(lambda g=g: check(lib.pis_debug_stream_probe(a.data_ptr(), b.data_ptr(), dst.data_ptr(), nf,
                                                                           0, g, st)), args.reps, fl, sink), g)
                   for g in PROBE_GRIDS) + (12 * nf,)

    for name, S, H, W in CONFIGS:
        rng = np.random.default_rng(S * 1000 + H)
        x = torch.from_numpy(rng.random((S, 1, H, W), dtype=np.float32)).to(dev)
        for tta in TTAS:
            p = pr.Predictor(model, tile=args.tile, overlap=args.overlap, tta=tta, batch_tiles=args.batch_tiles)
            plan = p.plan(H, W)
            J = plan.jobs(S)
            n, starts = pr.chunk_starts(J, args.batch_tiles)
            tt = plan.th * plan.tw
            say(f"\n{name}, tta {tta or 'none'}: tile {plan.th} x {plan.tw}, overlap {plan.ov}, {plan.Ky} x {plan.Kx} tiles, "
                f"{plan.Ns} symmetries, J = {J} jobs in {len(starts)} chunks of {n}; tile outputs {J * tt * 4 / 1e6:.1f} MB")
            src = x[:, 0].contiguous()
            tiles = torch.empty((n, 1, plan.th, plan.tw), device=dev)
            u = torch.rand((J, 1, plan.th, plan.tw), device=dev)
            prob = torch.empty((S, H, W), device=dev)
            mask = torch.empty((S, H, W), dtype=torch.uint8, device=dev)
            first = starts[len(starts) // 2]

            def gather(first=first):
                check(lib.pis_tile_gather(src.data_ptr(), _hip.PIS_CACHE_IMG_F32, H * W * 4, 0, S, H, W, plan.th, plan.tw,
                                          plan.ov, plan.sym_mask, first, n, tiles.data_ptr(), st))

            def blend():
                check(lib.pis_tile_blend(u.data_ptr(), S, H, W, plan.th, plan.tw, plan.ov, plan.sym_mask, 0.5,
                                         prob.data_ptr(), mask.data_ptr(), st))
            say("(a) per launch vs one pis_debug_stream_probe launch over the same bytes "
                f"(HIP events, median of {args.reps})")
            for what, fn, nbytes in (("tile_gather", gather, 2 * n * tt * 4), ("tile_blend", blend, J * tt * 4 + S * H * W * 5)):
                for state, fl in (("cold", flush), ("warm", None)):
                    k_ms = event_ms(fn, args.reps, fl, sink)
                    p_ms, grid, pbytes = probe_ms(nbytes, fl)
                    say(f"    {what:11s} {state}: {k_ms * 1e3:9.2f} us ({nbytes / k_ms / 1e6:7.1f} GB/s)   probe "
                        f"{p_ms * 1e3:9.2f} us (grid {grid}, {pbytes} B)   ratio {k_ms / p_ms:.2f}   "
                        f"[{nbytes} algorithmic bytes]")

            def forwards():
                with torch.no_grad():
                    for _ in starts:
                        model(tiles)

            def moves():
                for f in starts:
                    gather(f)
                blend()
            e2e = event_ms(lambda: p.predict_batch(x), args.e2e_reps)
            fwd = event_ms(forwards, args.e2e_reps)
            mv = event_ms(moves, args.e2e_reps)
            px = S * H * W
            say(f"(b) end to end (median of {args.e2e_reps}): predict_batch {e2e:9.3f} ms = {px / e2e / 1e3:8.1f} Mpixel/s, "
                f"{S / e2e * 1e3:7.2f} images/s;   the {len(starts)} forwards alone {fwd:9.3f} ms;   "
                f"ratio {e2e / fwd:.3f};   the {len(starts)} gathers + 1 blend alone {mv:8.3f} ms")
            eager = EagerTiling(plan, S, dev)
            with torch.no_grad():
                e_e2e = event_ms(lambda: eager.predict(model, src, args.batch_tiles), args.e2e_reps)

                def eager_moves():
                    for f in starts:
                        eager.gather(src, f, n)
                    eager.blend(u)
                e_mv = event_ms(eager_moves, args.e2e_reps)
                want = p.predict_batch(x)[0][:, 0]
                got = eager.predict(model, src, args.batch_tiles)[0]
            diff = float((want - got).abs().max())
            say(f"(c) eager torch, same tiling (median of {args.e2e_reps}): end to end {e_e2e:9.3f} ms "
                f"({e_e2e / e2e:.2f} x predict_batch);   its data movement alone {e_mv:9.3f} ms "
                f"({e_mv / mv:.1f} x the kernels');   max |eager - kernels| = {diff:.3g}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written {args.out}")


if __name__ == "__main__":
    main()
