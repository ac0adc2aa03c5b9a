"""Record the reference model's numbers that tests/test_model_parity.py and tests/test_train.py compare with.

    python tools/make_reference_golden.py --reference <dir holding the reference's modules.py>

runs the reference ``modules.py`` (fp32, CPU) on the tests' small configuration and writes
``tests/golden/reference_parity.npz``: its initial weights (state dict + the attention heads' parameters,
which the reference keeps in a plain list outside the state dict), one synthetic batch, the forward
outputs, the float64-weighted loss and every parameter gradient; and the same for one standalone
``GlobalAttentionHead``.  The tests load that file, so they need no copy of the reference.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from proteinbert_pytorch_replication_amd.data import SyntheticUniRefGO  # noqa: E402

CFG = dict(sequences_length=32, num_annotations=40, local_dim=16, global_dim=32, key_dim=8,
           num_heads=4, num_blocks=2)
OUT = os.path.join(ROOT, "tests", "golden", "reference_parity.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference's modules.py")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    import modules  # type: ignore

    rec = {}
    torch.manual_seed(0)
    ref = modules.ProteinBERT(device="cpu", **CFG)
    for k, v in ref.state_dict().items():
        rec["state/" + k] = v.detach().numpy().copy()
    rec["param_names"] = np.array([n for n, _ in ref.named_parameters()])
    for i, blk in enumerate(ref.proteinBERT_blocks):
        for j, h in enumerate(blk.global_attention_layer.global_attention_heads):
            for w in ("Wv", "Wk", "Wq"):
                rec[f"heads/{i}/{j}/{w}"] = getattr(h, w + "_parameter").detach().numpy().copy()
    X, Y, W = SyntheticUniRefGO(CFG["sequences_length"], CFG["num_annotations"], 3, "cpu", seed=1,
                                density=0.1, use_kernel=False).next_batch()
    for name, part in (("X", X), ("Y", Y), ("W", W)):
        for k, v in part.items():
            rec[f"batch/{name}/{k}"] = v.numpy().copy()
    with torch.no_grad():
        pl, pg = ref(X)
    rec["forward/local"], rec["forward/global"] = pl.numpy().copy(), pg.numpy().copy()
    W64 = {k: v.double() for k, v in W.items()}
    ce, bce = torch.nn.CrossEntropyLoss(reduction="none"), torch.nn.BCELoss(reduction="none")
    pl, pg = ref(X)
    loss = torch.mean(ce(pl.permute(0, 2, 1), Y["local"]) * W64["local"]) + \
        torch.mean(bce(pg, Y["global"].float()) * W64["global"])
    loss.backward()
    rec["loss"] = loss.detach().numpy().copy()
    for n, p in ref.named_parameters():
        rec["grad/" + n] = p.grad.numpy().copy()

    torch.manual_seed(3)
    head = modules.GlobalAttentionHead(16, 32, 8, 8, device="cpu")
    for k, v in head.state_dict().items():
        rec["head/state/" + k] = v.detach().numpy().copy()
    x = {"local": torch.randn(3, 20, 16) * 0.3, "global": torch.randn(3, 32) * 0.3}
    rec["head/x/local"], rec["head/x/global"] = x["local"].numpy().copy(), x["global"].numpy().copy()
    with torch.no_grad():
        rec["head/out"] = head(x).numpy().copy()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print(a.out, os.path.getsize(a.out), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
