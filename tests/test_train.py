"""Trainer: fused Adam vs torch Adam, checkpoint contract, resume, scheduler."""
import os

import pytest
import torch

from proteinbert_pytorch_replication_amd.models import ProteinBERT
from proteinbert_pytorch_replication_amd.data import SyntheticUniRefGO
from proteinbert_pytorch_replication_amd.train.optim import FusedAdam
from proteinbert_pytorch_replication_amd.train.arena import FlatArena
from proteinbert_pytorch_replication_amd.train.pretrain import pretrain
from proteinbert_pytorch_replication_amd.train.checkpoint import (REFERENCE_KEYS, load_checkpoint,
                                                                  load_reference_checkpoint)
from proteinbert_pytorch_replication_amd.train.schedulers import WarmupThenPlateau

CFG = dict(sequences_length=32, num_annotations=40, local_dim=16, global_dim=32, key_dim=8,
           num_heads=4, num_blocks=2)


def _model(seed=0):
    torch.manual_seed(seed)
    return ProteinBERT(backend="torch", **CFG)


def test_fused_adam_matches_torch_adam():
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(5, 7)), torch.nn.Parameter(torch.randn(13))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    fa = FusedAdam(ps, lr=1e-2, weight_decay=0.01)
    ta = torch.optim.Adam(ref, lr=1e-2, weight_decay=0.01)
    for it in range(5):
        grads = [torch.randn_like(p) for p in ps]
        fa.zero_grad()
        for p, g in zip(ps, grads):
            p.grad.copy_(g)
        fa.step()
        ta.zero_grad()
        for p, g in zip(ref, grads):
            p.grad = g.clone()
        ta.step()
    for p, r in zip(ps, ref):
        torch.testing.assert_close(p.detach(), r.detach(), rtol=1e-6, atol=1e-6)
    # state dict format is torch Adam's
    sd = fa.state_dict()
    ta2 = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1e-2)
    ta2.load_state_dict(sd)
    torch.testing.assert_close(ta2.state_dict()["state"][0]["exp_avg"], ta.state_dict()["state"][0]["exp_avg"])


def test_arena_views_and_alignment():
    m = _model()
    arena = FlatArena(m.parameters())
    for p, (o, n) in zip(arena.params, arena.offsets):
        assert o % 64 == 0
        assert p.data_ptr() == arena.data[o:].data_ptr()
    assert arena.grads_attached()
    m.zero_grad(set_to_none=True)
    assert not arena.grads_attached()
    arena.zero_grad()
    assert arena.grads_attached()


def test_scheduler_warmup_then_plateau():
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1.0)
    s = WarmupThenPlateau(opt, warmup_duration=4, patience=1)
    assert opt.param_groups[0]["lr"] == 0.0  # reference quirk Q8: lr starts at 0
    for i in range(4):
        s.step()
    assert abs(opt.param_groups[0]["lr"] - 1.0) < 1e-9
    s.step(1.0)
    s.step(1.0)
    s.step(1.0)
    assert opt.param_groups[0]["lr"] < 1.0


def test_pretrain_checkpoint_and_resume(tmp_path):
    m = _model()
    gen = SyntheticUniRefGO(CFG["sequences_length"], CFG["num_annotations"], 4, "cpu", seed=3, use_kernel=False)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    res = pretrain(m, gen, opt, max_batch_iterations=5, save_path=str(tmp_path), nb_iterations_checkpoint=2,
                   warmup_duration=2)
    assert len(res["train_loss"]) == 5
    ck = tmp_path / "proteinbert_pretraining_checkpoint_4.pt"
    assert ck.exists()
    blob = load_checkpoint(str(ck))
    for k in REFERENCE_KEYS:
        assert k in blob
    assert len(blob["model_state_dict"]) == len(m.state_dict())
    assert "attention_heads" in blob["extra_state"]
    # resume continues from iteration 4
    m2 = _model(seed=99)
    opt2 = torch.optim.Adam(m2.parameters(), lr=1e-3)
    res2 = pretrain(m2, gen, opt2, max_batch_iterations=6, save_path=str(tmp_path), nb_iterations_checkpoint=100,
                    warmup_duration=2, loaded_checkpoint=blob, final_save=False)
    assert len(res2["train_loss"]) == 2
    finals = [f for f in os.listdir(tmp_path) if f.startswith("proteinbert_pretrained_model_")]
    assert finals


def test_checkpoint_loads_into_reference(reference_golden, tmp_path):
    """The reference model is stood in for by its recorded state dict and ``named_parameters()`` order
    (tests/golden/reference_parity.npz): a strict ``load_state_dict`` needs exactly its keys and shapes,
    and its Adam takes our optimizer state only if the parameters line up one to one."""
    ref_state = {k[len("state/"):]: v for k, v in reference_golden.items() if k.startswith("state/")}
    m = _model()
    gen = SyntheticUniRefGO(CFG["sequences_length"], CFG["num_annotations"], 2, "cpu", seed=3, use_kernel=False)
    pretrain(m, gen, torch.optim.Adam(m.parameters(), lr=1e-3), max_batch_iterations=2,
             save_path=str(tmp_path), nb_iterations_checkpoint=1, warmup_duration=1, final_save=False)
    blob = load_checkpoint(str(tmp_path / "proteinbert_pretraining_checkpoint_1.pt"))
    ours = blob["model_state_dict"]
    assert list(ours.keys()) == list(ref_state.keys())
    for k, v in ref_state.items():
        assert ours[k].shape == v.shape and ours[k].dtype == v.dtype, k
    ref_params = [torch.nn.Parameter(torch.empty_like(ref_state[n])) for n in reference_golden["param_names"]]
    ref_opt = torch.optim.Adam(ref_params, lr=1e-3)
    ref_opt.load_state_dict(blob["optimizer_state_dict"])
    for p, st in zip(ref_params, ref_opt.state_dict()["state"].values()):
        assert st["exp_avg"].shape == p.shape
    # and a reference-produced checkpoint loads into ours (heads re-drawn)
    m2 = _model(seed=5)
    load_reference_checkpoint(m2, {"model_state_dict": ref_state})
    torch.testing.assert_close(m2.state_dict()["local_embedding.weight"], ref_state["local_embedding.weight"])


def test_pretrain_profile_window_writes_trace(tmp_path):
    """a torch.profiler window over steps 2-3 -> Chrome trace + kernel table."""
    m = _model()
    gen = SyntheticUniRefGO(CFG["sequences_length"], CFG["num_annotations"], 4, "cpu", seed=1, use_kernel=False)

    class _Loader:
        def __iter__(self):
            while True:
                yield gen.next_batch()

    res = pretrain(m, _Loader(), torch.optim.Adam(m.parameters(), lr=1e-3), max_batch_iterations=4,
                   save_path=str(tmp_path), nb_iterations_checkpoint=100, warmup_duration=2, final_save=False,
                   profile_steps="2:2")
    trace = res["profile_trace"]
    assert os.path.exists(trace) and os.path.getsize(trace) > 0
    assert os.path.exists(trace.replace(".json", ".txt"))
    assert "steps2-3" in trace
