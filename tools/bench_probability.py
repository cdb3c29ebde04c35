"""Probability table: device path (pis_probability_table) against the host path, one read probe over
the same bytes and one sample_counts call, at 8 x 512^2 and 64 x 128^2.

    python tools/bench_probability.py                 # writes profiles/probability_metrics.txt
    python tools/bench_probability.py --out FILE --reps 30

Per shape and input it times ``evaluate.probability_table`` per call with HIP events: the first call
of the process at that shape ("cold": the workspace comes fresh from the caching allocator and the
kernels are loaded on first use) and the median of --reps warm calls, each the two launches plus the
allocation of workspace, table and extra. A call is short enough for the host's enqueue to show in
that figure, so the two launches alone are timed as well: ``pis_probability_table`` on preallocated
buffers, --batch calls back to back between two events, median over --reps such batches, per call.
That form is repeated for every value of pis_tune key 52 (the kernel forms: end bins by ballot +
popcount, four histograms per block instead of two, no merging of a lane's equal neighbours), side
by side.

Yardsticks at the same shape: the host path (numpy, one thread, host clock); ONE
``pis_debug_stream_probe`` read launch over the same p and t (8 B per pixel), best over its grid
sizes, timed like the launches; one ``sample_counts`` call (the fused loss forward that yields the
Dice / IoU counters), per call like the first figure.

Inputs: sigmoid of Gaussian-filtered noise (a soft prediction), the same field saturated to {0, 1}
(what a trained phase-field-regularised network gives: both end bins), and a constant 0.3 (one
interior bin: the LDS atomics' worst case); targets are a second blurred field cut at its middle.
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
from physics_informed_image_segmentation_amd.metrics import sample_counts  # noqa: E402

SHAPES = ((8, 512, 512), (64, 128, 128))
VARIANTS = ((0, "default: every bin by LDS atomics, 2 histograms, merged runs"), (1, "end bins by ballot + popcount"),
            (2, "4 histograms per block"), (3, "end-bin ballots, 4 histograms"), (4, "no merging of equal neighbours"),
            (5, "end-bin ballots, no merging"), (6, "4 histograms, no merging"),
            (7, "end-bin ballots, 4 histograms, no merging"))


def make_inputs(B, H, W):
    from scipy import ndimage
    rng = np.random.default_rng(42)

    def field():
        return np.stack([ndimage.gaussian_filter(rng.standard_normal((H, W)), 3.0) for _ in range(B)])
    soft = (1.0 / (1.0 + np.exp(-12.0 * field()))).astype(np.float32)
    t = (field() > 0).astype(np.float32)
    return {"blurred": torch.from_numpy(soft), "saturated": torch.from_numpy((soft > 0.5).astype(np.float32)),
            "constant 0.3": torch.full((B, H, W), 0.3)}, torch.from_numpy(t)


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return out, (e0, e1)


def per_call_ms(fn, reps):
    """Median / min / max over reps calls, one event pair per call."""
    for _ in range(3):
        fn()
    pairs = [_events(fn)[1] for _ in range(reps)]
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in pairs)
    return t[len(t) // 2], t[0], t[-1]


def batched_us(fn, reps, batch):
    """Median over reps of (batch back-to-back calls between two events) / batch, in microseconds."""
    def run():
        for _ in range(batch):
            fn()
    run()
    pairs = [_events(run)[1] for _ in range(reps)]
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in pairs) / batch * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probability_metrics.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_probability: needs the GPU")
    torch.set_num_threads(1)
    lib = _hip.lib()
    st = _hip.stream_handle()
    lines = [f"probability_table (pis_probability_table) on {torch.cuda.get_device_name(0)}: per call = events around "
             f"one evaluate.probability_table call, median of {args.reps}; launches = {args.batch} C calls on "
             f"preallocated buffers between two events, median of {args.reps}, per call"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def check(rc):
        if rc != 0:
            raise RuntimeError(lib.pis_last_error().decode())

    for B, H, W in SHAPES:
        nbytes = lib.pis_probability_ws(B, H, W)
        say(f"\n{B} x {H} x {W}: {8 * B * H * W / 1e6:.1f} MB read, workspace {nbytes} bytes, "
            f"{-(-H * W // ev.PROB_BLOCK_PIXELS) * B} blocks")
        preds, t = make_inputs(B, H, W)
        tc = t.cuda()
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        table = torch.empty((B, 2, 1025, 2), dtype=torch.int64, device="cuda")
        extra = torch.empty((B, 4), dtype=torch.int64, device="cuda")
        partial = torch.empty(16384, device="cuda")
        for name, p in preds.items():
            pc = p.cuda()
            torch.cuda.synchronize()
            (tab, ext), (e0, e1) = _events(lambda: ev.probability_table(pc, tc))
            torch.cuda.synchronize()
            cold = e0.elapsed_time(e1)
            med, lo, hi = per_call_ms(lambda: ev.probability_table(pc, tc), args.reps)
            smed, slo, shi = per_call_ms(lambda: sample_counts(pc, tc, 0.5), args.reps)
            t0 = time.perf_counter()
            host = ev.probability_table(p, t, backend="host")
            host_ms = (time.perf_counter() - t0) * 1e3
            ok = torch.equal(tab.cpu(), host[0]) and torch.equal(ext.cpu(), host[1])
            probe_us, grid = min((batched_us(lambda g=g: check(lib.pis_debug_stream_probe(
                pc.data_ptr(), tc.data_ptr(), 0, pc.numel(), partial.data_ptr(), g, st)), args.reps, args.batch), g)
                for g in (256, 512, 1024, 2048, 4096, 8192))
            say(f"  {name}: per call cold {cold:.3f} ms, warm median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max "
                f"{hi * 1e3:.1f}); host path {host_ms:.1f} ms ({host_ms / med:.0f} x); sample_counts per call warm "
                f"median {smed * 1e3:.1f} us (min {slo * 1e3:.1f}, max {shi * 1e3:.1f}); read probe {probe_us:.1f} us "
                f"(grid {grid}); matches host: {ok}")
            assert ok
            base = None
            for v, what in VARIANTS:
                prev = lib.pis_tune(_hip.PIS_TUNE_PROB_VARIANT, v)
                try:
                    us = batched_us(lambda: check(lib.pis_probability_table(
                        pc.data_ptr(), tc.data_ptr(), B, H, W, table.data_ptr(), extra.data_ptr(), ws.data_ptr(),
                        nbytes, st)), args.reps, args.batch)
                    torch.cuda.synchronize()
                    same = torch.equal(table.cpu(), host[0]) and torch.equal(extra.cpu(), host[1])
                finally:
                    lib.pis_tune(_hip.PIS_TUNE_PROB_VARIANT, prev)
                base = us if base is None else base
                say(f"    launches, key 52 = {v} ({what}): {us:.1f} us = {us / probe_us:.2f} x read probe, "
                    f"{us / base:.2f} x default, {8 * B * H * W / us / 1e6:.2f} TB/s; matches host: {same}")
                assert same
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written {args.out}")


if __name__ == "__main__":
    main()
