"""Time the reference-semantics local head at the headline shapes: the one-launch route vs the five-pass
form (ops/global_track.py local_head_forward), both in one process, alternated round by round.
B <= 1024 flips LHEAD_FUSED; 1024 < B <= 2048 flips LHEAD_FUSED_MAX_B between 2048 and 1024 (the parent's
routing).
    python tools/ubench/lhead_b.py [--B 2048 --L 512 --rounds 5 --iters 20]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from proteinbert_pytorch_replication_amd.ops import global_track as gt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=2048)
ap.add_argument("--L", type=int, default=512)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda")
torch.manual_seed(0)
B, L, V = a.B, a.L, 26
h = torch.randn(B, L, 128, device=dev).to(torch.bfloat16)
wo, bo = torch.randn(V, 128, device=dev) * 0.1, torch.randn(V, device=dev)
y = torch.randint(0, V, (B, L), device=dev)
w = (torch.rand(B, L, device=dev) < 0.9).float()

if B <= 1024:
    modes = {"one-launch": ("LHEAD_FUSED", True), "five-pass": ("LHEAD_FUSED", False)}
else:
    modes = {"one-launch": ("LHEAD_FUSED_MAX_B", 2048), "five-pass": ("LHEAD_FUSED_MAX_B", 1024)}


def run():
    loss = torch.zeros(1, device=dev)
    return gt.local_head_forward(h, wo, bo, y, w, loss), loss


res, times = {}, {k: [] for k in modes}
for rnd in range(a.rounds + 1):                       # round 0 warms both routes up
    for name, (attr, val) in modes.items():
        saved = getattr(gt, attr)
        setattr(gt, attr, val)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            out = run()
        e1.record()
        torch.cuda.synchronize()
        setattr(gt, attr, saved)
        res[name] = out
        if rnd:
            times[name].append(e0.elapsed_time(e1) / a.iters * 1000)
for name, t in times.items():
    print(f"B={B} L={L} {name:10s}: min {min(t):.1f} max {max(t):.1f} us per call "
          f"(rounds: {' '.join(f'{x:.1f}' for x in t)})", flush=True)
(d1, z1, _), l1 = res["one-launch"]
(d2, z2, _), l2 = res["five-pass"]
print("max |dh diff|:", float((d1.float() - d2.float()).abs().max()), " max |dz diff|:",
      float((z1.float() - z2.float()).abs().max()), " loss:", float(l1), float(l2))
