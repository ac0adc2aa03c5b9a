"""FusedAdam with parameter groups and decoupled weight decay on the CPU: against torch.optim.Adam / AdamW
with the same groups, state dicts both ways, ``param_groups_for``, ``pretrain()`` with a two-group AdamW,
ZeRO-1 over two gloo ranks and the ``finetune`` CLI with an encoder learning rate of its own."""
import json
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from proteinbert_pytorch_replication_amd.data import SyntheticUniRefGO
from proteinbert_pytorch_replication_amd.models import ProteinBERT
from proteinbert_pytorch_replication_amd.train.checkpoint import load_checkpoint
from proteinbert_pytorch_replication_amd.train.optim import FusedAdam, make_optimizer, param_groups_for
from proteinbert_pytorch_replication_amd.train.pretrain import pretrain

CFG = dict(sequences_length=32, num_annotations=40, local_dim=16, global_dim=32, key_dim=8,
           num_heads=4, num_blocks=2)
# three groups that differ in every per-group value; the second does not move (lr = 0)
HP = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),
      dict(lr=0.0, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1),
      dict(lr=3e-3, betas=(0.95, 0.9), eps=1e-7, weight_decay=0.0)]


def _mlp(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(7, 13), torch.nn.Tanh(), torch.nn.Linear(13, 70), torch.nn.Tanh(),
                               torch.nn.Linear(70, 3))


def _split(model, n_groups):
    """Interleaved groups (parameter i goes to group i % n), so neighbours in the arena differ in group."""
    ps = list(model.parameters())
    return [dict(params=ps[k::n_groups], **HP[k]) for k in range(n_groups)]


def _train(model, opt, steps, seed=1):
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        x = torch.randn(16, 7, generator=gen)
        opt.zero_grad()
        model(x).square().mean().backward()
        opt.step()


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("n_groups", [2, 3])
def test_groups_match_torch(n_groups, decoupled):
    ma, mb = _mlp(), _mlp()
    fa = FusedAdam(_split(ma, n_groups), decoupled_weight_decay=decoupled)
    ta = (torch.optim.AdamW if decoupled else torch.optim.Adam)(_split(mb, n_groups))
    assert len(fa.param_groups) == n_groups
    assert all(g["decoupled_weight_decay"] is decoupled for g in fa.param_groups)
    frozen = [p.detach().clone() for p in fa.param_groups[1]["params"]]
    _train(ma, fa, 5)
    _train(mb, ta, 5)
    for p, r in zip(ma.parameters(), mb.parameters()):
        torch.testing.assert_close(p.detach(), r.detach(), rtol=1e-6, atol=1e-6)     # tests/test_train.py:29-42
    moved = [not torch.equal(p.detach(), q) for p, q in zip(fa.param_groups[1]["params"], frozen)]
    assert not any(moved)              # lr = 0: neither rule moves a parameter (AdamW's 1 - lr * wd is 1)
    assert any(not torch.equal(p.detach(), q.detach()) for p, q in zip(ma.parameters(), _mlp().parameters()))


def test_decoupled_per_group_override():
    """decoupled_weight_decay as a default and overridden in one group: a mixed Adam / AdamW optimizer."""
    ma, mb = _mlp(), _mlp()
    ga, gb = _split(ma, 2), _split(mb, 2)
    ga[1].update(lr=2e-3, decoupled_weight_decay=True)
    gb[1].update(lr=2e-3, decoupled_weight_decay=True)
    fa, ta = FusedAdam(ga), torch.optim.Adam(gb)
    assert [g["decoupled_weight_decay"] for g in fa.param_groups] == [False, True]
    _train(ma, fa, 5)
    _train(mb, ta, 5)
    for p, r in zip(ma.parameters(), mb.parameters()):
        torch.testing.assert_close(p.detach(), r.detach(), rtol=1e-6, atol=1e-6)


def test_one_group_hparam_block_unchanged():
    """One group: the device block is the 8 floats it was, and a group dict of one is the same optimizer."""
    ma, mb = _mlp(), _mlp()
    fa = FusedAdam(ma.parameters(), lr=1e-2, weight_decay=0.01)
    fb = FusedAdam([dict(params=list(mb.parameters()))], lr=1e-2, weight_decay=0.01)
    assert fa._hp_dev.numel() == 8 and fb._hp_dev.numel() == 8
    _train(ma, fa, 3)
    _train(mb, fb, 3)
    assert torch.equal(fa.arena.data, fb.arena.data) and torch.equal(fa._hp_dev, fb._hp_dev)
    assert FusedAdam(_split(_mlp(), 3))._hp_dev.numel() == 24


def test_state_dict_round_trip_with_adamw():
    """FusedAdam -> torch.optim.AdamW -> FusedAdam after 3 steps: torch's numbering, and the next step is the
    same on all three."""
    ma, mb, mc = _mlp(), _mlp(), _mlp()
    fa = FusedAdam(_split(ma, 2), decoupled_weight_decay=True)
    _train(ma, fa, 3)
    sd = fa.state_dict()
    sizes = [len(g["params"]) for g in fa.param_groups]
    assert len(sd["param_groups"]) == 2
    assert [g["params"] for g in sd["param_groups"]] == [list(range(sizes[0])), list(range(sizes[0], sum(sizes)))]
    assert sorted(sd["state"]) == list(range(sum(sizes)))
    mb.load_state_dict(ma.state_dict())
    ta = torch.optim.AdamW(_split(mb, 2))
    ref = torch.optim.AdamW(_split(_mlp(), 2)).state_dict()
    assert [g["params"] for g in ref["param_groups"]] == [g["params"] for g in sd["param_groups"]]
    ta.load_state_dict(sd)
    mc.load_state_dict(ma.state_dict())
    fc = FusedAdam(_split(mc, 2), decoupled_weight_decay=False)
    fc.load_state_dict(ta.state_dict())
    assert fc.step_count == 3 and all(g["decoupled_weight_decay"] for g in fc.param_groups)
    assert [g["lr"] for g in fc.param_groups] == [g["lr"] for g in fa.param_groups]
    for m, o in ((ma, fa), (mb, ta), (mc, fc)):
        _train(m, o, 1, seed=7)
    for p, q, r in zip(ma.parameters(), mb.parameters(), mc.parameters()):
        assert torch.equal(p.detach(), r.detach())                       # fused -> torch -> fused: identical
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-6, atol=1e-6)
    sa, sc = fa.state_dict(), fc.state_dict()
    for i in sa["state"]:
        assert torch.equal(sa["state"][i]["exp_avg_sq"], sc["state"][i]["exp_avg_sq"])


def test_group_mismatch_and_limits_raise():
    m = _mlp()
    fa = FusedAdam(_split(m, 2))
    _train(m, fa, 1)
    with pytest.raises(ValueError):
        FusedAdam(_split(_mlp(), 3)).load_state_dict(fa.state_dict())             # another number of groups
    ps = list(_mlp().parameters())
    with pytest.raises(ValueError):                                              # the same number, other sizes
        FusedAdam([dict(params=ps[:1]), dict(params=ps[1:])], lr=1e-3).load_state_dict(fa.state_dict())
    with pytest.raises(ValueError):
        FusedAdam(_mlp().parameters(), lr=1e-3).load_state_dict(fa.state_dict())
    many = [torch.nn.Parameter(torch.zeros(3)) for _ in range(17)]
    with pytest.raises(ValueError):
        FusedAdam([dict(params=[p]) for p in many], lr=1e-3)
    assert len(FusedAdam([dict(params=[p]) for p in many[:16]], lr=1e-3).param_groups) == 16
    with pytest.raises(ValueError):
        fa.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(3))]))


def test_block_table_follows_the_arena():
    m = _mlp()
    fa = FusedAdam(_split(m, 3))
    a = fa.arena
    table = fa._block_group.tolist()
    assert len(table) == a.numel // 64
    want = {id(p): gi for gi, g in enumerate(fa.param_groups) for p in g["params"]}
    for p, (o, n) in zip(a.params, a.offsets):
        blocks = table[o // 64:(o + n + 63) // 64]
        assert blocks and set(blocks) == {want[id(p)]}                           # the padding belongs to its parameter
    assert len(set(table)) == 3


def test_param_groups_for():
    torch.manual_seed(0)
    model = ProteinBERT(backend="torch", **CFG)
    groups = param_groups_for(model, 1e-3, weight_decay=0.1,
                              lr_scale={"proteinBERT_blocks.": 0.1, "proteinBERT_blocks.1.": 0.5})
    named = {id(p): n for n, p in model.named_parameters() if p.requires_grad}
    seen = [id(p) for g in groups for p in g["params"]]
    assert sorted(seen) == sorted(named) and len(set(seen)) == len(seen)         # each exactly once
    assert all(g["params"] for g in groups) and len(groups) == 6
    for g in groups:
        names = [named[id(p)] for p in g["params"]]
        if g["weight_decay"] == 0.0:
            assert all("bias" in n or "norm" in n for n in names), names
        else:
            assert g["weight_decay"] == 0.1 and not any("bias" in n or "norm" in n for n in names), names
        scale = {0.5 if n.startswith("proteinBERT_blocks.1.") else 0.1 if n.startswith("proteinBERT_blocks.") else 1.0
                 for n in names}
        assert len(scale) == 1 and g["lr"] == pytest.approx(1e-3 * scale.pop(), rel=1e-12)
    assert any("local_norm_1.weight" in named[id(p)] for g in groups if g["weight_decay"] == 0.0 for p in g["params"])
    again = param_groups_for(model, 1e-3, weight_decay=0.1,
                             lr_scale={"proteinBERT_blocks.1.": 0.5, "proteinBERT_blocks.": 0.1})
    assert [[id(p) for p in g["params"]] for g in again] == [[id(p) for p in g["params"]] for g in groups]
    assert [(g["lr"], g["weight_decay"]) for g in again] == [(g["lr"], g["weight_decay"]) for g in groups]
    # no weight decay, no scale: one group; an empty no_decay list: everything decays
    assert len(param_groups_for(model, 1e-3)) == 1
    assert [g["weight_decay"] for g in param_groups_for(model, 1e-3, 0.1, no_decay=())] == [0.1]
    # make_optimizer keeps the arena in the model's reverse-registration order whatever the grouping
    opt = make_optimizer(model, groups=groups, decoupled_weight_decay=True)
    assert [id(p) for p in opt.arena.params] == [id(p) for p in model.parameters()][::-1]
    assert len(opt.param_groups) == 6 and all(g["decoupled_weight_decay"] for g in opt.param_groups)


def _pb(seed=0):
    torch.manual_seed(seed)
    return ProteinBERT(backend="torch", **CFG)


def _two_group_adamw(model):
    groups = param_groups_for(model, 1e-3, weight_decay=0.1)
    assert len(groups) == 2
    groups[1]["lr"] = 5e-4
    return torch.optim.AdamW(groups, betas=(0.9, 0.99))


def _gen(skip=0):
    gen = SyntheticUniRefGO(CFG["sequences_length"], CFG["num_annotations"], 4, "cpu", seed=3, use_kernel=False)
    for _ in range(skip):
        gen.next_batch()
    return gen


def test_pretrain_fuses_two_group_adamw_and_resumes(tmp_path):
    m = _pb()
    res = pretrain(m, _gen(), _two_group_adamw(m), max_batch_iterations=6, save_path=str(tmp_path / "a"),
                   nb_iterations_checkpoint=3, warmup_duration=4, final_save=False)
    opt = res["optimizer"]
    assert type(opt) is FusedAdam and len(opt.param_groups) == 2
    assert all(g["decoupled_weight_decay"] for g in opt.param_groups)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.1, 0.0]
    assert [g["betas"] for g in opt.param_groups] == [(0.9, 0.99)] * 2
    assert [id(p) for p in opt.arena.params] == [id(p) for p in m.parameters()][::-1]
    # the warmup scales both groups' rates: after 6 steps of a 4-step warmup both are back at their base
    assert [g["lr"] for g in opt.param_groups] == pytest.approx([1e-3, 5e-4], rel=1e-12)
    blob = load_checkpoint(str(tmp_path / "a" / "proteinbert_pretraining_checkpoint_3.pt"))
    saved = blob["optimizer_state_dict"]["param_groups"]
    assert [g["lr"] for g in saved] == pytest.approx([0.75e-3, 0.75 * 5e-4], rel=1e-12)   # step 3 of 4, both groups
    m2 = _pb(seed=99)
    res2 = pretrain(m2, _gen(skip=3), _two_group_adamw(m2), max_batch_iterations=6, save_path=str(tmp_path / "b"),
                    nb_iterations_checkpoint=100, warmup_duration=4, loaded_checkpoint=blob, final_save=False)
    assert len(res2["train_loss"]) == 3 and res2["optimizer"].step_count == 6
    for (n, p), q in zip(m.named_parameters(), m2.parameters()):
        assert torch.equal(p.detach(), q.detach()), n


def test_pretrain_one_group_adam_is_todays_optimizer():
    m = _pb()
    res = pretrain(m, _gen(), torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=0.01), max_batch_iterations=1,
                   save_path=".", nb_iterations_checkpoint=100, warmup_duration=1, final_save=False)
    opt = res["optimizer"]
    assert type(opt) is FusedAdam and len(opt.param_groups) == 1 and opt._hp_dev.numel() == 8
    assert opt._decoupled_mask() == 0
    m2 = _pb()
    keep = torch.optim.Adam(m2.parameters(), lr=1e-3, amsgrad=True)
    res = pretrain(m2, _gen(), keep, max_batch_iterations=1, save_path=".", nb_iterations_checkpoint=100,
                   warmup_duration=1, final_save=False)
    assert res["optimizer"] is keep                                              # amsgrad stays with PyTorch


# ---- two gloo ranks: ZeRO-1 with groups against the unsharded update (after tests/test_zero.py) ----------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _zero_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from proteinbert_pytorch_replication_amd.parallel import dist as pdist
    from proteinbert_pytorch_replication_amd.parallel.ddp import BucketedAllReduce
    from proteinbert_pytorch_replication_amd.parallel.zero import ZeroFusedAdam
    from proteinbert_pytorch_replication_amd.train.arena import FlatArena
    from proteinbert_pytorch_replication_amd.train.step import PretrainStep
    pdist.init_distributed(device="cpu")
    ma, mb = _pb(), _pb()

    def groups(model):
        gs = param_groups_for(model, 1e-2, weight_decay=0.1, lr_scale={"proteinBERT_blocks.": 0.5})
        gs[0].update(betas=(0.8, 0.99), eps=1e-6)
        return gs

    oa = make_optimizer(ma, groups=groups(ma), decoupled_weight_decay=True)
    ddp = BucketedAllReduce(oa.arena, bucket_mb=0.01)
    sa = PretrainStep(ma, oa, ddp)                      # the overlapped path: finish_and_step with four groups
    ob = ZeroFusedAdam(groups(mb), arena=FlatArena(mb.parameters()), decoupled_weight_decay=True)
    assert len(oa.param_groups) == 4 and len(ob.param_groups) == 4
    assert ob.lo % 64 == 0 and (ob.lo > 0) == (rank > 0)      # rank 1's launch starts inside the block table
    sb = PretrainStep(mb, ob)
    gen = SyntheticUniRefGO(CFG["sequences_length"], CFG["num_annotations"], 4, "cpu", seed=50 + rank,
                            use_kernel=False)
    for _ in range(3):
        batch = gen.next_batch()
        sa(*batch)
        sb(*batch)
    perr = max((pa - pb).abs().max().item() for pa, pb in zip(ma.parameters(), mb.parameters()))
    sda, sdb = oa.state_dict(), ob.state_dict()
    same_groups = [g["params"] for g in sda["param_groups"]] == [g["params"] for g in sdb["param_groups"]]
    serr = max(max((sda["state"][i][k] - sdb["state"][i][k]).abs().max().item() for k in ("exp_avg", "exp_avg_sq"))
               for i in sda["state"])
    oc = ZeroFusedAdam(groups(mb), arena=ob.arena, decoupled_weight_decay=True)
    oc.load_state_dict(sdb)
    rt = max((oc.exp_avg - ob.exp_avg).abs().max().item(), (oc.exp_avg_sq - ob.exp_avg_sq).abs().max().item())
    torch.save({"perr": perr, "serr": serr, "rt": rt, "steps": oc.step_count, "same_groups": same_groups,
                "n_groups": len(sdb["param_groups"]), "overlapped": sa.overlapped_optimizer()},
               os.path.join(out_dir, f"r{rank}.pt"))
    pdist.destroy()


def test_zero1_groups_match_unsharded(tmp_path):
    world = 2
    mp.start_processes(_zero_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, start_method="spawn",
                       join=True)
    for r in range(world):
        e = torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True)
        assert e["perr"] < 1e-6 and e["serr"] < 1e-6, e                           # the bounds of tests/test_zero.py
        assert e["rt"] == 0.0 and e["steps"] == 3 and e["same_groups"] and e["n_groups"] == 4, e
        assert e["overlapped"], e


# ---- the finetune CLI ---------------------------------------------------------------------------------------
SMALL = ["model.sequences_length=32", "model.num_annotations=40", "model.local_dim=16", "model.global_dim=32",
         "model.key_dim=8", "model.num_blocks=1", "train.batch_size=4", "kernel.backend=torch", "kernel.dtype=fp32"]


def test_finetune_cli_encoder_lr(tmp_path, capsys, monkeypatch):
    from proteinbert_pytorch_replication_amd.cli import train as cli_train
    from proteinbert_pytorch_replication_amd.train import finetune as ft
    start = {}
    real = ft.finetune

    def spy(model, *a, **kw):
        start.update({n: p.detach().clone() for n, p in model.named_parameters()})
        return real(model, *a, **kw)

    monkeypatch.setattr(ft, "finetune", spy)
    res = cli_train.finetune_main(["--preset", "cfg1_cpu_smoke", *SMALL, f"train.save_path={tmp_path}", "--epochs", "1",
                                   "--synthetic-samples", "16", "--unfreeze", "--lr", "1e-3", "--encoder-lr", "1e-4"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(out["train_loss"]) == 1
    opt = res["optimizer"]
    assert type(opt) is FusedAdam and len(opt.param_groups) == 2
    assert sorted(g["lr"] for g in opt.param_groups) == [1e-4, 1e-3]
    lr_of = {id(p): g["lr"] for g in opt.param_groups for p in g["params"]}
    ordered = opt.arena.params[::-1]                   # the arena holds model.parameters(), reversed
    assert len(ordered) == len(start) == len(lr_of)
    moved = {"encoder": 0, "head": 0}
    for (n, before), p in zip(start.items(), ordered):
        part = "encoder" if n.startswith("encoder.") else "head"
        assert before.shape == p.shape and lr_of[id(p)] == (1e-4 if part == "encoder" else 1e-3), n
        moved[part] += int(not torch.equal(before, p.detach()))
    assert moved["encoder"] > 0 and moved["head"] > 0, moved


def test_pretrain_cli_builds_groups_from_the_config(tmp_path, capsys):
    from proteinbert_pytorch_replication_amd.cli.train import pretrain_main
    from proteinbert_pytorch_replication_amd.config import OptimConfig
    assert OptimConfig().decoupled_weight_decay is False and OptimConfig().no_decay_norm_bias is False
    args = ["--preset", "cfg1_cpu_smoke", *SMALL, "optim.warmup_duration=2", f"train.save_path={tmp_path}",
            "train.max_batch_iterations=2", "train.nb_iterations_checkpoint=100"]
    res = pretrain_main(args + ["optim.weight_decay=0.01", "optim.no_decay_norm_bias=true",
                                "optim.decoupled_weight_decay=true", "--resume", "none"])
    opt = res["optimizer"]
    assert type(opt) is FusedAdam and [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0]
    assert all(g["decoupled_weight_decay"] for g in opt.param_groups)
    res = pretrain_main(args + ["optim.weight_decay=0.01", "--resume", "none"])                      # the defaults: one group, as before
    opt = res["optimizer"]
    assert len(opt.param_groups) == 1 and opt._decoupled_mask() == 0 and opt.param_groups[0]["weight_decay"] == 0.01
    capsys.readouterr()


def test_finetune_cli_default_is_one_group(tmp_path, capsys):
    from proteinbert_pytorch_replication_amd.cli.train import finetune_main
    res = finetune_main(["--preset", "cfg1_cpu_smoke", *SMALL, f"train.save_path={tmp_path}", "--epochs", "1",
                         "--synthetic-samples", "16", "--unfreeze"])
    capsys.readouterr()
    opt = res["optimizer"]
    assert len(opt.param_groups) == 1 and opt._decoupled_mask() == 0 and opt.param_groups[0]["weight_decay"] == 0.0
