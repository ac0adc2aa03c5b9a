"""The grouped Adam launch against the flat one: ``pbx_adam_flat`` and ``pbx_adam_flat_groups`` (G = 2 and G = 8)
on the paper-config model's arena, with the bf16 shadow and the device step counter in use, alternated round by
round in one process.  The block tables change group at every parameter boundary of the model (parameter i is in
group i % G); every second group decays its weights AdamW's way.  Device events around runs of back-to-back
launches; the medians and the spread of the rounds go to ``--out``.

    python tools/adam_groups_bench.py [--preset cfg2_paper_l512] [--rounds 15] [--launches 300] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from proteinbert_pytorch_replication_amd.config import get_preset  # noqa: E402
from proteinbert_pytorch_replication_amd.models import build_model  # noqa: E402
from proteinbert_pytorch_replication_amd.ops import _lib  # noqa: E402
from proteinbert_pytorch_replication_amd.train.optim import FusedAdam  # noqa: E402


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg2_paper_l512")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "adam_groups_ubench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_groups_bench needs a GPU")
    cfg = get_preset(a.preset)
    torch.manual_seed(0)
    model = build_model(cfg.model, device="cuda", backend="hip")
    opt = FusedAdam(model.parameters(), lr=1e-5, weight_decay=0.01)
    arena = opt.arena
    n = arena.numel
    assert opt.shadow is not None
    arena.grad.copy_(torch.randn(n, device="cuda") * 1e-3)
    opt._step_dev.fill_(100.0)
    st = _lib.stream_ptr(arena.data.device)
    ptrs = (arena.data.data_ptr(), arena.grad.data_ptr(), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(),
            opt.shadow.data_ptr(), n)
    one = opt._hparam_values()

    def grouped(G):
        hp = torch.tensor([v for k in range(G) for v in (one[0] * (1 + k),) + one[1:]], dtype=torch.float32,
                          device="cuda")
        table = torch.zeros(n // 64, dtype=torch.uint8)
        for i, (o, k) in enumerate(arena.offsets):
            table[o // 64:(o + k + 63) // 64] = i % G
        table = table.cuda()
        mask = sum(1 << k for k in range(1, G, 2))
        return lambda: _lib.call("pbx_adam_flat_groups", *ptrs, hp.data_ptr(), G, mask, table.data_ptr(), None,
                                 opt._step_dev.data_ptr(), st)

    opt.prepare()
    runs = {"pbx_adam_flat": lambda: _lib.call("pbx_adam_flat", *ptrs, opt._hp_dev.data_ptr(), None,
                                               opt._step_dev.data_ptr(), st),
            "pbx_adam_flat_groups G=2": grouped(2), "pbx_adam_flat_groups G=8": grouped(8)}
    for fn in runs.values():                          # warm-up: code objects, clocks
        window_us(fn, 20)
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            times[k].append(window_us(fn, a.launches))
    assert bool(torch.isfinite(arena.data).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    flat = med["pbx_adam_flat"]
    gbytes = n * 30 / 1e9                              # p, m, v read and written, g read, the shadow written
    lines = [f"adam_groups_bench: preset {a.preset}, arena {n} fp32 elements in {len(arena.offsets)} segments "
             f"({gbytes:.3f} GB moved per launch at 30 B/element), bf16 shadow and step_dev in use",
             f"{a.rounds} rounds, the three launchers alternated, {a.launches} back-to-back launches per window "
             f"(device events), us per launch", ""]
    for k, v in times.items():
        lines.append(f"{k:28s} median {med[k]:8.2f}  min {min(v):8.2f}  max {max(v):8.2f}  "
                     f"spread (max - min) / median {100 * (max(v) - min(v)) / med[k]:5.2f} %  "
                     f"{gbytes / (med[k] * 1e-6) / 1e3:6.3f} TB/s  vs flat {100 * (med[k] / flat - 1):+6.2f} %")
    lines += ["", "rounds (us): " + "; ".join(f"{k}: " + " ".join(f"{x:.2f}" for x in v) for k, v in times.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
