"""Cost of one physics-diagnostics call (nbx_diagnostics: the all-pairs potential energy plus the O(n) sums) against one
default force step of the same context, per n: ms of each and the ratio.  The design target is a ratio of at most 1 at
n = 262144 fp32 (<= 2 % of a 50-step print window); tests/test_diagnostics_gpu.py gates it loosely at 3.
usage: python tools/diag_cost.py [n ...]   (GPU box, repo root)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(nbx, n, precision=32, steps=10, calls=5):
    """{'step_ms', 'diag_ms', 'ratio'}: wall time per default force step (host clock around steps that end in a
    synchronisation) and per diagnostics call (each synchronises), both warmed up."""
    with nbx.Context(n, precision, device=0) as c:
        c.upload(nbx.initial_conditions(n, precision))
        c.step(2)
        c.diagnostics()
        t0 = time.perf_counter()
        c.step(steps)
        step_s = (time.perf_counter() - t0) / steps
        t0 = time.perf_counter()
        for _ in range(calls):
            c.diagnostics()
        diag_s = (time.perf_counter() - t0) / calls
    return {"step_ms": 1e3 * step_s, "diag_ms": 1e3 * diag_s, "ratio": diag_s / step_s}


def main():
    sys.path.insert(0, os.path.join(ROOT, "nbody-demo-2023_amd"))
    import nbx
    sizes = [int(x) for x in sys.argv[1:]] or [16384, 65536, 262144, 1048576]
    print("%9s %14s %14s %8s" % ("n", "step ms", "diag ms", "ratio"))
    for n in sizes:
        r = measure(nbx, n)
        print("%9d %14.4f %14.4f %8.3f" % (n, r["step_ms"], r["diag_ms"], r["ratio"]), flush=True)


if __name__ == "__main__":
    main()
