"""What the clipped / guarded optimizer step costs at the benchmark network's size.

Times, in ONE process on one GPU, at n = 12 346 468 parameters:
  plain     FusedAdam.step()                                            (one mi_adam_step launch)
  guarded   FusedAdam(max_grad_norm=1, skip_nonfinite=True).step()      (mi_grad_norm: two launches; mi_adam_step_guarded: one)
  norm      mi_grad_norm alone
  parent    mi_adam_step of another build of the library (--parent-lib PATH, e.g. the parent commit's), called through ctypes directly:
            shows the plain path unchanged
Device events around every step, the first --warmup steps discarded, the median of --steps (>= 50).

    python scripts/optim_step_timing.py [--steps 100] [--warmup 20] [--parent-lib PATH] [--out profiles/optim_step_timing.txt]

--ema times instead, ALTERNATING in one process over --rounds rounds of --steps steps each, plain and guarded:
  step          FusedAdam.step() without an average                         (7 array passes: 4 read, 3 written)
  fused         FusedAdam(ema_decay=0.999).step(): mi_adam_step_ema         (9: one more read, one more written)
  step + lerp_  the first, followed by ema.lerp_(theta, 1 - decay) of torch   (10: the separate launch re-reads the new weights)
and prints each variant's median over all rounds with the spread of the per-round medians.

    python scripts/optim_step_timing.py --ema [--steps 50] [--rounds 5] [--out profiles/ema_step_timing.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from matinvent_amd import _lib  # noqa: E402
from matinvent_amd.build import build  # noqa: E402
from matinvent_amd.cspnet import _ptr, _stream  # noqa: E402
from matinvent_amd.optim import GRAD_STATS, FusedAdam  # noqa: E402

N = 12346468


def timed(fn, steps, warmup):
    ms = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ms), min(ms)


def ema_rows(args):
    """The three forms of a step with an average, plain and guarded, alternating round by round; rows of (name, median, min, per-round medians)."""
    torch.manual_seed(0)
    grad = torch.randn(N, device="cuda")

    def fresh(**kw):
        p = torch.nn.Parameter(torch.randn(N, device="cuda"))
        p.grad = grad
        return p, FusedAdam([p], lr=1e-4, **kw)

    variants = []
    for tag, guard in (("", {}), ("guarded ", dict(max_grad_norm=1.0, skip_nonfinite=True))):
        _, a = fresh(**guard)
        _, b = fresh(ema_decay=0.999, **guard)
        p, c = fresh(**guard)
        avg = p.detach().clone()

        def separate(c=c, p=p, avg=avg):
            c.step()
            avg.lerp_(p.detach(), 1.0 - 0.999)
        variants += [(tag + "step", a.step), (tag + "fused step + average (mi_adam_step_ema)", b.step), (tag + "step + torch lerp_", separate)]
    samples = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, fn in variants:
            ms = []
            for i in range((args.warmup if r == 0 else 3) + args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b) * 1e3)
            samples[name].append(ms[-args.steps:])
    return [(name, statistics.median([x for r in samples[name] for x in r]), min(x for r in samples[name] for x in r),
             [statistics.median(r) for r in samples[name]]) for name, _ in variants]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ema", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.steps >= 50
    build(verbose=False)
    if args.ema:
        rows = ema_rows(args)
        lines = [f"optimizer step with a weight average at n = {N} on {torch.cuda.get_device_name(0)}; device events, {args.rounds} alternating rounds of "
                 f"{args.steps} steps, one process; median (min) [per-round medians]"]
        lines += [f"  {name:<58s} {med:8.1f} us  ({lo:.1f})  [{', '.join(f'{x:.1f}' for x in per)}]" for name, med, lo, per in rows]
        for k in (0, 3):
            lines.append(f"  {rows[k][0]:<14s} fused / step = {rows[k + 1][1] / rows[k][1]:.3f} (traffic alone: 9 / 7 = 1.286);  "
                         f"separate / step = {rows[k + 2][1] / rows[k][1]:.3f} (10 / 7 = 1.429);  fused / separate = {rows[k + 1][1] / rows[k + 2][1]:.3f} (0.900)")
        text = "\n".join(lines)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    lib = _lib.load()
    torch.manual_seed(0)
    grad = torch.randn(N, device="cuda")
    rows = []

    def fresh(**kw):
        p = torch.nn.Parameter(torch.randn(N, device="cuda"))
        p.grad = grad
        return FusedAdam([p], lr=1e-4, **kw)

    plain = fresh()
    rows.append(("plain FusedAdam.step", *timed(plain.step, args.steps, args.warmup)))
    guarded = fresh(max_grad_norm=1.0, skip_nonfinite=True)
    rows.append(("guarded step (clip on, skip on)", *timed(guarded.step, args.steps, args.warmup)))
    s = dict(zip(GRAD_STATS, guarded.grad_stats().tolist()))
    assert s["applied_steps"] == s["clipped_steps"] == args.steps + args.warmup and s["skipped_steps"] == 0, s
    state, work = torch.zeros(16, dtype=torch.int32, device="cuda"), torch.empty(lib.mi_optim_workspace_bytes(N) // 4, device="cuda")
    norm = lambda: _lib.check(lib.mi_grad_norm(_ptr(grad), N, 1.0, 1.0, 1, 1e-4, 0.9, 0.999, _ptr(state), _ptr(work), _stream()))
    rows.append(("mi_grad_norm alone", *timed(norm, args.steps, args.warmup)))
    if args.parent_lib:
        old = C.CDLL(args.parent_lib)
        old.mi_adam_step.restype, old.mi_adam_step.argtypes = _lib.SIGNATURES["mi_adam_step"]
        p, m, v = torch.randn(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        step = [0]

        def parent():
            step[0] += 1
            assert old.mi_adam_step(_ptr(p), _ptr(grad), _ptr(m), _ptr(v), N, step[0], 1e-4, 0.9, 0.999, 1e-8, 1.0, _stream()) == 0

        rows.append((f"plain mi_adam_step of {os.path.basename(args.parent_lib)}", *timed(parent, args.steps, args.warmup)))
        rows.append(("plain FusedAdam.step (again)", *timed(plain.step, args.steps, args.warmup)))
    lines = [f"optimizer step at n = {N} on {torch.cuda.get_device_name(0)}; device events, {args.warmup} warm-up steps discarded, "
             f"median (min) of {args.steps} steps, one process"]
    lines += [f"  {name:<52s} {med:8.1f} us  ({lo:.1f})" for name, med, lo in rows]
    lines.append(f"  guarded / plain = {rows[1][1] / rows[0][1]:.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
