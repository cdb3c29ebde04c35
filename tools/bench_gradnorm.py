"""Global-norm gradient clipping and the non-finite step guard: what they cost, at the U-Net's size.

    python tools/bench_gradnorm.py                  # all parts -> profiles/grad_clip.txt
    python tools/bench_gradnorm.py --part a --out - # the norm pass only, to stdout

(a) ``pis_grad_sumsq`` (the segmented sum of squares + its finalize launch) over the model's own
segment table and a gradient arena of the model's size, timed with HIP events, median of --reps:
cold (a 1 GiB read between launches, bench.py's protocol) and warm (back to back). Beside it ONE
``pis_debug_stream_probe`` launch in its reducing form (a read of two arrays, one partial per block)
over as many floats as make its bytes equal the gradients the norm pass reads, same protocol, best
over the probe's grid sizes.

(b) ``pis_adamw_step_clipped`` against ``pis_adamw_step`` over the same arena, the two launches
interleaved repetition by repetition, cold and warm.

(c) The C2 step (8 x 512^2, Stage-II loss, forward + loss + backward + optimizer) with
``AdamW(max_grad_norm=, skip_nonfinite=True)`` against the plain ``AdamW``: two optimizers on ONE
shared model (separately allocated models differ by placement alone), alternating in
one process, --rounds rounds of --steps steps each after a warm-up; host clock around a
synchronised block of steps. The margin a difference has to leave to count is the plain rounds'
own spread. No bar is set: the figures are the record.
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_loader import event_ms, events_ms  # noqa: E402


def _check(lib, rc):
    if rc != 0:
        raise RuntimeError(lib.pis_last_error().decode())


def part_a_b(parts, reps, say):
    from physics_informed_image_segmentation_amd import UNet, _hip
    lib = _hip.lib()
    st = _hip.stream_handle()
    entries = UNet(1, 1, 64).arena_entries()
    arena_n = UNet(1, 1, 64).arena.numel()
    lens = [n for _, _, n in entries]
    live = sum(lens)
    flush = torch.ones(256 << 20, device="cuda")  # 1 GiB
    sink = torch.empty((), device="cuda")
    g = torch.randn(arena_n, device="cuda") * 1e-3
    off = torch.tensor([o for _, o, _ in entries], dtype=torch.int64, device="cuda")
    ln = torch.tensor(lens, dtype=torch.int64, device="cuda")
    sumsq = torch.zeros(len(lens), dtype=torch.float64, device="cuda")
    record = torch.zeros(2, dtype=torch.float64, device="cuda")
    stats = torch.zeros(_hip.PIS_GRADNORM_NSTATS, dtype=torch.float64, device="cuda")
    ws_bytes = lib.pis_grad_sumsq_ws(len(lens), live)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

    def norm():
        _check(lib, lib.pis_grad_sumsq(g.data_ptr(), off.data_ptr(), ln.data_ptr(), len(lens), 1.0, 1.0,
                                       _hip.PIS_GRADNORM_SKIP_NONFINITE, sumsq.data_ptr(), record.data_ptr(),
                                       stats.data_ptr(), ws.data_ptr(), ws_bytes, st))
    if "a" in parts:
        say(f"(a) pis_grad_sumsq (sum of squares + finalize) over {len(lens)} segments, {live} gradients "
            f"({4 * live / 1e6:.1f} MB read; arena {arena_n} floats) vs one pis_debug_stream_probe launch reading the "
            f"same bytes (HIP events, median of {reps})")
        nf = -(-live // 8) * 4  # floats per probe array: two arrays read, n % 4 == 0
        a, b = torch.ones(nf, device="cuda"), torch.ones(nf, device="cuda")
        partial = torch.empty(8192, device="cuda")

        def probe(grid):
            _check(lib, lib.pis_debug_stream_probe(a.data_ptr(), b.data_ptr(), 0, nf, partial.data_ptr(), grid, st))
        for state, fl in (("cold", flush), ("warm", None)):
            k_ms = event_ms(norm, reps, fl, sink)
            p_ms, grid = min((event_ms(lambda gr=gr: probe(gr), reps, fl, sink), gr) for gr in (512, 1024, 2048, 4096, 8192))
            say(f"  {state}:  grad_sumsq {k_ms * 1e3:8.2f} us ({4 * live / k_ms / 1e6:7.1f} GB/s)   "
                f"probe {p_ms * 1e3:8.2f} us (grid {grid}, {8 * nf} B)   ratio {k_ms / p_ms:.2f}")
    if "b" in parts:
        say(f"(b) pis_adamw_step_clipped vs pis_adamw_step over {arena_n} floats (p, g, m, v; launches "
            f"interleaved, HIP events, median of {reps})")
        norm()
        p, m, v = (torch.zeros(arena_n, device="cuda") for _ in range(3))
        head = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), arena_n, 0.0, 0.9, 0.999, 1e-8, 0.0, 0.0, 1.0,
                1.0)
        fns = {"plain": lambda: _check(lib, lib.pis_adamw_step(*head, st)),
               "clipped": lambda: _check(lib, lib.pis_adamw_step_clipped(*head, record.data_ptr(), st))}
        for state, fl in (("cold", flush), ("warm", None)):
            ms = events_ms(fns, reps, fl, sink)
            say(f"  {state}:  adamw_step {ms['plain'] * 1e3:8.2f} us   adamw_step_clipped {ms['clipped'] * 1e3:8.2f} us   "
                f"clipped / plain {ms['clipped'] / ms['plain']:.3f}")


def part_c(rounds, steps, say):
    from physics_informed_image_segmentation_amd import AdamW, DiceBCEPDELoss, UNet
    from physics_informed_image_segmentation_amd.dataset import disc_sample
    dev = torch.device("cuda", torch.cuda.current_device())
    rounds = max(rounds, 5)
    gen = torch.Generator().manual_seed(42)
    imgs, masks = zip(*[disc_sample(512, 512, gen) for _ in range(8)])
    x, t = torch.stack(imgs).to(dev), torch.stack(masks).to(dev)
    torch.manual_seed(42)
    net = UNet(1, 1, 64).to(dev).train()
    crit = DiceBCEPDELoss(pde_weight=1e-4, phase_field_weight=1e-4, diffusion_coeff=5.0, reaction_threshold=0.5,
                          epsilon=0.05).to(dev)
    opts = {"clipping off": AdamW(net.parameters(), lr=1e-5, weight_decay=1e-5),
            "clipping on": AdamW(net.parameters(), lr=1e-5, weight_decay=1e-5, max_grad_norm=1.0,
                                 skip_nonfinite=True)}

    def run(opt, n):
        for _ in range(n):
            opt.zero_grad()
            _, loss = net.forward_with_loss(x, t, crit)
            loss.backward()
            opt.step()
    say(f"(c) C2 step (8 x 512^2, Stage II) ms, AdamW(max_grad_norm=1.0, skip_nonfinite=True) vs AdamW() on one "
        f"shared model, alternating in one process: 1 warm-up + {rounds} timed rounds of {steps} steps each")
    times = {k: [] for k in opts}
    for r in range(rounds + 1):
        for name, opt in opts.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(opt, steps)
            torch.cuda.synchronize()
            if r:
                times[name].append((time.perf_counter() - t0) / steps * 1e3)
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        say(f"    {name:13s} median {med[name]:7.3f} ms   minimum {min(ts):7.3f} ms   (rounds: "
            + ", ".join(f"{v:.3f}" for v in ts) + ")")
    ts = times["clipping off"]
    spread = (max(ts) - min(ts)) / statistics.median(ts)
    diff = med["clipping on"] / med["clipping off"] - 1.0
    say(f"    on / off = {1.0 + diff:.4f} ({(med['clipping on'] - med['clipping off']) * 1e3:+.1f} us per step, median); "
        f"the off rounds' own spread (max - min) / median = {spread:.4f}: the difference is "
        f"{'inside' if abs(diff) <= spread else 'OUTSIDE'} it")
    gs = opts["clipping on"].pop_grad_stats()
    say(f"    the clipping optimizer saw {gs['steps']} steps: {gs['clipped_steps']} clipped, {gs['skipped_steps']} skipped, "
        f"mean norm {gs['norm_sum'] / max(gs['finite_steps'], 1):.4g}, max {gs['norm_max']:.4g}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=["a", "b", "c", "all"], default="all")
    ap.add_argument("--reps", type=int, default=50, help="timed launches per kernel figure")
    ap.add_argument("--rounds", type=int, default=6, help="timed rounds per optimizer (at least 5)")
    ap.add_argument("--steps", type=int, default=20, help="steps per round")
    ap.add_argument("--out", default=None, help="report file ('-': stdout only; default: profiles/grad_clip.txt)")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = str(Path(__file__).resolve().parent.parent / "profiles" / "grad_clip.txt")
    if not torch.cuda.is_available():
        raise SystemExit("bench_gradnorm.py: needs the MI355X (no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/bench_gradnorm.py --part {args.part} --reps {args.reps} --rounds {args.rounds} --steps {args.steps}   "
        f"[{torch.cuda.get_device_name(0)}, torch {torch.__version__}]")
    parts = ("a", "b", "c") if args.part == "all" else (args.part,)
    if "a" in parts or "b" in parts:
        part_a_b(parts, args.reps, say)
    if "c" in parts:
        part_c(args.rounds, args.steps, say)
    if args.out != "-":
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
