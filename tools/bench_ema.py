"""EMA weight averaging inside the fused AdamW step: what it costs, at the U-Net's size.

    python tools/bench_ema.py                  # all parts -> profiles/ema.txt
    python tools/bench_ema.py --part a --out - # the launches only, to stdout

(a) ``pis_adamw_step_ema`` (p, g, m, v, e read; p, m, v, e written: nine arena passes) over an arena
of the model's size against ``pis_adamw_step`` (seven passes) and against the unfused form it
replaces, ``pis_adamw_step`` followed by ``ema.lerp_(arena, w)`` (ten passes, two launches). Beside
them ONE ``pis_debug_stream_probe`` launch in its copying form (two arrays read, one written) over as
many floats as make its bytes equal the fused launch's, best over the probe's grid sizes. All
interleaved repetition by repetition, cold (a 1 GiB read between launches, bench.py's protocol) and
warm (back to back), HIP events, median of --reps.

(b) ``pis_arena_exchange`` (two arrays read, two written) against the probe moving the same bytes.

(c) The C2 step (8 x 512^2, Stage-II loss, forward + loss + backward + optimizer) with
``AdamW(ema_decay=0.999)`` against the plain ``AdamW``: two optimizers on ONE shared model (separately
allocated models differ by placement alone), alternating in one process, --rounds rounds
of --steps steps each after a warm-up; host clock around a synchronised block of steps. The margin a
difference has to leave to count is the off rounds' own spread. No bar is set: the figures are the
record.
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_loader import events_ms  # noqa: E402

PROBE_GRIDS = (1024, 2048, 4096, 8192)


def _check(lib, rc):
    if rc != 0:
        raise RuntimeError(lib.pis_last_error().decode())


def part_a_b(parts, reps, say):
    from physics_informed_image_segmentation_amd import UNet, _hip
    lib = _hip.lib()
    st = _hip.stream_handle()
    arena_n = UNet(1, 1, 64).arena.numel()
    flush = torch.ones(256 << 20, device="cuda")  # 1 GiB
    sink = torch.empty((), device="cuda")
    w = 0.001

    def probe_fns(nbytes):
        """One probe launch per grid size moving nbytes: a and b read, dst written."""
        nf = -(-nbytes // 48) * 4  # floats per array, n % 4 == 0
        a, b, dst = (torch.ones(nf, device="cuda") for _ in range(3))
        keep = (a, b, dst)
        return {f"probe{gr}": (lambda gr=gr, keep=keep: _check(lib, lib.pis_debug_stream_probe(
            keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), nf, 0, gr, st))) for gr in PROBE_GRIDS}, 12 * nf

    def best_probe(ms):
        return min((v, int(k[5:])) for k, v in ms.items() if k.startswith("probe"))

    if "a" in parts:
        say(f"(a) pis_adamw_step_ema vs pis_adamw_step vs pis_adamw_step + ema.lerp_(arena, w) over {arena_n} floats "
            f"({4 * arena_n / 1e6:.1f} MB per array; the fused launch moves {36 * arena_n / 1e6:.1f} MB) vs one "
            f"pis_debug_stream_probe launch moving the same bytes (interleaved, HIP events, median of {reps})")
        g = torch.randn(arena_n, device="cuda") * 1e-3
        p, m, v = (torch.zeros(arena_n, device="cuda") for _ in range(3))
        e = torch.zeros(arena_n, device="cuda")
        head = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
        tail = (arena_n, 0.0, 0.9, 0.999, 1e-8, 0.0, 0.0, 1.0, 1.0)

        def plain():
            _check(lib, lib.pis_adamw_step(*head, *tail, st))

        def unfused():
            plain()
            e.lerp_(p, w)
        fns = {"plain": plain,
               "fused": lambda: _check(lib, lib.pis_adamw_step_ema(*head, e.data_ptr(), *tail, w, 0, st)),
               "unfused": unfused}
        probes, pbytes = probe_fns(36 * arena_n)
        fns.update(probes)
        for state, fl in (("cold", flush), ("warm", None)):
            ms = events_ms(fns, reps, fl, sink)
            p_ms, grid = best_probe(ms)
            say(f"  {state}:  adamw_step {ms['plain'] * 1e3:8.2f} us   adamw_step_ema {ms['fused'] * 1e3:8.2f} us "
                f"({36 * arena_n / ms['fused'] / 1e6:7.1f} GB/s)   adamw_step + lerp_ {ms['unfused'] * 1e3:8.2f} us   "
                f"probe {p_ms * 1e3:8.2f} us (grid {grid}, {pbytes} B)")
            say(f"         fused / plain {ms['fused'] / ms['plain']:.3f}   fused / unfused {ms['fused'] / ms['unfused']:.3f}   "
                f"fused / probe {ms['fused'] / p_ms:.3f}")
        del probes
    if "b" in parts:
        say(f"(b) pis_arena_exchange over two arrays of {arena_n} floats ({16 * arena_n / 1e6:.1f} MB moved) vs one "
            f"pis_debug_stream_probe launch moving the same bytes (interleaved, HIP events, median of {reps})")
        a, b = torch.zeros(arena_n, device="cuda"), torch.ones(arena_n, device="cuda")
        fns = {"exchange": lambda: _check(lib, lib.pis_arena_exchange(a.data_ptr(), b.data_ptr(), arena_n, st))}
        probes, pbytes = probe_fns(16 * arena_n)
        fns.update(probes)
        for state, fl in (("cold", flush), ("warm", None)):
            ms = events_ms(fns, reps, fl, sink)
            p_ms, grid = best_probe(ms)
            say(f"  {state}:  arena_exchange {ms['exchange'] * 1e3:8.2f} us ({16 * arena_n / ms['exchange'] / 1e6:7.1f} GB/s)   "
                f"probe {p_ms * 1e3:8.2f} us (grid {grid}, {pbytes} B)   ratio {ms['exchange'] / p_ms:.3f}")


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
    opts = {"ema off": AdamW(net.parameters(), lr=1e-5, weight_decay=1e-5),
            "ema on": AdamW(net.parameters(), lr=1e-5, weight_decay=1e-5, ema_decay=0.999)}

    def run(opt, n):
        for _ in range(n):
            opt.zero_grad()
            _, loss = net.forward_with_loss(x, t, crit)
            loss.backward()
            opt.step()
    say(f"(c) C2 step (8 x 512^2, Stage II) ms, AdamW(ema_decay=0.999) vs AdamW() on one shared model, alternating "
        f"in one process: 1 warm-up + {rounds} timed rounds of {steps} steps each")
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
        say(f"    {name:8s} median {med[name]:7.3f} ms   minimum {min(ts):7.3f} ms   (rounds: "
            + ", ".join(f"{v:.3f}" for v in ts) + ")")
    ts = times["ema off"]
    spread = (max(ts) - min(ts)) / statistics.median(ts)
    diff = med["ema on"] / med["ema off"] - 1.0
    say(f"    on / off = {1.0 + diff:.4f} ({(med['ema on'] - med['ema off']) * 1e3:+.1f} us per step, median); "
        f"the off rounds' own spread (max - min) / median = {spread:.4f}: the difference is "
        f"{'inside' if abs(diff) <= spread else 'OUTSIDE'} it")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=["a", "b", "c", "all"], default="all")
    ap.add_argument("--reps", type=int, default=50, help="timed launches per kernel figure")
    ap.add_argument("--rounds", type=int, default=6, help="timed rounds per optimizer (at least 5)")
    ap.add_argument("--steps", type=int, default=20, help="steps per round")
    ap.add_argument("--out", default=None, help="report file ('-': stdout only; default: profiles/ema.txt)")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = str(Path(__file__).resolve().parent.parent / "profiles" / "ema.txt")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema.py: needs the MI355X (no CPU fallback)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/bench_ema.py --part {args.part} --reps {args.reps} --rounds {args.rounds} --steps {args.steps}   "
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
