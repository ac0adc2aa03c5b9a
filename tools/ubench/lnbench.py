"""Stand-alone timing of the LayerNorm / local-MLP kernels of csrc/ln.hip (pbx_ln_linear_fwd,
pbx_ln2_linear_bwd, pbx_ln1_finalize) at the headline shape, for several builds of the kernel library in ONE
process, rounds interleaved (build variants with tools/ubench/build_flags.sh):

    python tools/ubench/lnbench.py parent=tools/ubench/abl/libpbx_parent.so new=<...>/libpbx_hip.so \
        [--B 2048] [--L 512] [--rounds 7] [--calls 10]

Prints per kernel and build the median / min us per call over the rounds and bytes / time with the bytes the
kernel has to move (fwd: s1 in, pre_l + s2 out; bwd: dh2, s2, pre_l, s1 in, dh1 out; fin: dh1, s1 in, ds1 out).
Inputs are random (not a consistent forward): the kernels' time does not depend on the values.
"""
import argparse
import ctypes
import statistics
import sys

import torch

sys.path.insert(0, ".")
from proteinbert_pytorch_replication_amd.ops import _lib  # noqa: E402

CH, PB, BM1, EPS = 128, 32, 128, 1e-5


def load(path):
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for name, args in _lib.launchers().items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = args, ctypes.c_int
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="name=path")
    ap.add_argument("--B", type=int, default=2048)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    B, L = a.B, a.L
    dev = torch.device("cuda:0")
    _ = torch.zeros(1, device=dev)
    libs = [(s.split("=", 1)[0], load(s.split("=", 1)[1])) for s in a.libs]
    st = _lib.stream_ptr(dev)
    T1, T2, TS1 = (L + BM1 - 1) // BM1, (L + PB - 1) // PB, (L + 1) // 2
    act = lambda: torch.randn(B, L, CH, device=dev).to(torch.bfloat16)   # noqa: E731
    s1, pre, s2, dh2, dh1, ds1 = act(), act(), act(), act(), act(), act()
    f32 = lambda *s: torch.randn(*s, device=dev)   # noqa: E731
    g1, be1, g2, bl = 1 + 0.1 * f32(L, CH), 0.1 * f32(L, CH), 1 + 0.1 * f32(L, CH), 0.1 * f32(CH)
    wl = (f32(CH, CH) / CH ** 0.5).to(torch.bfloat16)
    # (mean, M2) partials of unit-variance tiles, backward partials of zero mean
    st1 = torch.stack([torch.zeros(B, T1, device=dev), torch.full((B, T1), float(BM1 * CH), device=dev)], 2).contiguous()
    st2 = torch.empty(B, T2, 2, device=dev)
    sums2 = torch.zeros(B, T2, 2, device=dev)
    sums1 = torch.empty(B, TS1, 2, device=dev)
    consts, dgb = torch.empty(B, 8, device=dev), torch.zeros(B, CH, device=dev)
    dg = [torch.zeros(L, CH, device=dev) for _ in range(4)]
    dwl, dbl = torch.zeros(CH, CH, device=dev), torch.zeros(CH, device=dev)
    rows = libs[0][1].pbx_ln2_bwd_slab_rows(B, L, 0)
    slab = torch.empty(rows * (CH * CH + CH), device=dev)
    p = lambda t: t.data_ptr()   # noqa: E731

    def fwd(lib):
        return lib.pbx_ln_linear_fwd(p(s1), p(st1), T1, BM1, p(g1), p(be1), p(wl), p(bl), p(pre), p(s2), p(st2), B, L,
                                     EPS, st)

    def bwd(lib):
        # consts_ready after the first call: the kernel alone, as in the step (the consts kernel is 10 us)
        return lib.pbx_ln2_linear_bwd(p(dh2), p(s2), p(st2), p(sums2), T2, p(g2), p(pre), p(s1), p(st1), T1, BM1,
                                      p(g1), p(be1), p(wl), p(consts), p(dh1), p(sums1), p(dg[0]), p(dg[1]), p(dg[2]),
                                      p(dg[3]), p(dwl), p(dbl), p(dgb), B, L, EPS, p(slab), rows, 0, 0, bwd.ready, st)

    bwd.ready = 0

    def fin(lib):
        return lib.pbx_ln1_finalize(p(dh1), p(s1), p(st1), T1, BM1, p(sums1), TS1, p(g1), p(ds1), p(dgb), B, L, EPS, 0,
                                    st)

    act_mb = B * L * CH * 2 / 1e6
    kernels = [("ln_linear_fwd", fwd, 3 * act_mb), ("ln2_linear_bwd", bwd, 5 * act_mb), ("ln1_finalize", fin, 3 * act_mb)]
    for _, lib in libs:                       # warm-up: code objects, attributes, st2 / consts written
        for _, fn, _ in kernels:
            rc = fn(lib)
            assert rc == 0, rc
    torch.cuda.synchronize()
    bwd.ready = 1
    times = {(k, n): [] for k, _, _ in kernels for n, _ in libs}
    for _ in range(a.rounds):
        for kname, fn, _ in kernels:
            for n, lib in libs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    rc = fn(lib)
                e1.record()
                e1.synchronize()
                assert rc == 0, rc
                times[(kname, n)].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    print(f"B={B} L={L} rounds={a.rounds} calls/round={a.calls} (us per call, launch gaps included)")
    for kname, _, mb in kernels:
        for n, _ in libs:
            t = times[(kname, n)]
            med, mn = statistics.median(t), min(t)
            print(f"{kname:16s} {n:10s} median {med:7.1f} min {mn:7.1f} max {max(t):7.1f}   {mb:6.0f} MB  "
                  f"{mb / med:5.2f} TB/s at the median")


if __name__ == "__main__":
    main()
