"""Optimizer parameter groups, host side (no GPU): patterns -> range table, the library's range planner and argument checks,
the checkpoint round trip of EMA weights and patterns, the exported torch.optim.AdamW state, train.py's keys."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from optim_groups_ref import TorchGroups, match, small_cfg


def _flat(segmem=0):
    from mrmt3.params import FlatParams
    return FlatParams(small_cfg(), segmem)


# ---- patterns -> ranges ----------------------------------------------------------------------------------------------
def test_patterns_become_merged_ranges_in_flat_order():
    from mrmt3.params import ParamGroups
    flat = _flat()
    keys = list(flat.shapes)
    g = ParamGroups(keys, frozen=["encoder.*"], no_decay=["*layer_norm.weight"])
    assert g.frozen == match(keys, ["encoder.*"]) and "proj.weight" in g.frozen            # the alias encoder.embed_tokens
    assert "decoder.final_layer_norm.weight" in g.no_decay and not g.trivial
    rng = g.ranges(flat, 0.01)
    # sorted, disjoint, 4-aligned, and exactly the trainable elements with the right hyper-parameters
    cover = np.zeros(flat.numel, np.int8)
    prev = 0
    for a, b, wd, sc in rng:
        assert a >= prev and b > a and a % 4 == 0 and b % 4 == 0 and sc == 1.0 and wd in (0.0, 0.01)
        cover[a:b] = 1 if wd == 0.01 else 2
        prev = b
    for k, off in flat.offsets.items():
        want = 0 if k in g.frozen else (2 if k in g.no_decay else 1)
        assert (cover[off:off + flat.numel_of(k)] == want).all(), k
    # neighbours of equal hyper-parameters are merged: no two touching ranges agree, and there are far fewer ranges than tensors
    for x, y in zip(rng, rng[1:]):
        assert not (x[1] == y[0] and x[2:] == y[2:])
    n_train = sum(1 for k in keys if k not in g.frozen)
    assert len(rng) < n_train / 2, (len(rng), n_train)
    # all-trainable, no option: trivial; one no-decay tensor in the middle: three ranges around it
    assert ParamGroups(keys).trivial
    one = ParamGroups(keys, no_decay=["decoder.block.0.layer.0.layer_norm.weight"]).ranges(flat, 0.01)
    assert len(one) == 3 and one[0][0] == 0 and one[2][1] == flat.numel and one[1][2] == 0.0 and one[1][1] - one[1][0] == 512
    sc = ParamGroups(keys, lr_scale={"decoder.*": 0.5, "lm_head.weight": 2.0})
    assert sc.hyper("lm_head.weight", 0.01) == (0.01, 2.0) and sc.hyper("decoder.final_layer_norm.weight", 0.01) == (0.01, 0.5)
    assert sc.hyper("proj.weight", 0.01) == (0.01, 1.0)


def test_pattern_errors():
    from mrmt3.params import ParamGroups, ema_decay_option
    keys = list(_flat().shapes)
    with pytest.raises(ValueError, match="encodr"):
        ParamGroups(keys, frozen=["encodr.*"])
    with pytest.raises(ValueError, match="no_decay.*nothing_here"):
        ParamGroups(keys, no_decay=["*layer_norm.weight", "nothing_here"])
    with pytest.raises(ValueError, match="lr_scale.*zzz"):
        ParamGroups(keys, lr_scale={"zzz*": 0.5})
    with pytest.raises(ValueError, match="lr_scale"):
        ParamGroups(keys, lr_scale={"decoder.*": -1.0})
    with pytest.raises(ValueError, match="every parameter is frozen"):
        ParamGroups(keys, frozen=["*"])
    with pytest.raises(ValueError, match="list of patterns"):
        ParamGroups(keys, frozen="encoder.*")
    for bad in (0.0, 1.0, -0.1, 1.5, True, "0.9", float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            ema_decay_option(bad)
    assert ema_decay_option(None) is None and ema_decay_option(0.999) == 0.999


# ---- the library's planner and argument checks (host code) ----------------------------------------------------------------
def test_range_planner_table_and_errors():
    from mrmt3 import lib
    t = lib.OptRanges([(0, 4, 0.01, 1.0), (8, 1000, 0.0, 0.5), (1000, 1024, 0.01, 1.0)], 1024)
    assert t.n_trainable == 4 + 992 + 24 and len(t) == 3
    rec = np.frombuffer(t.host.numpy().tobytes(), dtype=np.dtype([("begin4", "<i8"), ("start", "<i8"), ("wd", "<f4"),
                                                                    ("sc", "<f4"), ("end4", "<i8")]))
    assert len(rec) == 4 and rec["begin4"].tolist()[:3] == [0, 2, 250] and rec["end4"].tolist()[:3] == [1, 250, 256]
    assert rec["start"].tolist() == [0, 1, 249, 255]                                   # prefix of 16-byte groups + the total
    assert rec["wd"].tolist()[:3] == [np.float32(0.01), 0.0, np.float32(0.01)] and rec["sc"].tolist()[:3] == [1.0, 0.5, 1.0]
    for bad, why in (([(0, 8, 0, 1), (4, 12, 0, 1)], "sorted and disjoint"), ([(8, 12, 0, 1), (0, 4, 0, 1)], "sorted and disjoint"),
                     ([(0, 6, 0, 1)], "multiples of 4"), ([(2, 8, 0, 1)], "multiples of 4"), ([(8, 8, 0, 1)], "empty"),
                     ([(0, 2048, 0, 1)], "past the buffer"), ([(0, 8, -1.0, 1)], "weight_decay"),
                     ([(0, 8, 0, float("nan"))], "lr_scale"), ([], "nothing to step")):
        with pytest.raises(ValueError, match=why):
            lib.OptRanges(bad, 1024)


def test_step_entry_points_check_their_arguments_before_any_launch():
    """Every call below fails its host-side checks (code 1, a message); the pointers are never dereferenced."""
    L = __import__("mrmt3.lib", fromlist=["load"]).load()
    p = C.c_void_p(0x1000)
    tab = C.c_void_p(0x2000)

    def step(ema=None, ema_decay=0.0, stat=None, clip=0.0, n=1024, nr=1, ntr=1024, table=tab):
        return L.mrmt3_adamw_step(p, p, p, p, ema, n, table, nr, ntr, p, p, 0.9, 0.999, 1e-8, 0.01, 1.0, ema_decay, stat, clip,
                                  None, None)

    for kw, why in ((dict(ema_decay=0.9), b"needs an ema buffer"), (dict(ema=p, ema_decay=0.0), b"ema buffer was given"),
                    (dict(ema=p, ema_decay=1.0), b"outside (0, 1)"), (dict(ema=p, ema_decay=-0.5), b"outside (0, 1)"),
                    (dict(ema=p, ema_decay=float("nan")), b"outside (0, 1)"), (dict(clip=-1.0), b"clip_value"),
                    (dict(clip=0.5), b"needs stat_dev"), (dict(n=1022), b"bad args"), (dict(nr=0), b"ranges"),
                    (dict(nr=-1), b"ranges"), (dict(nr=1 << 20), b"ranges"),
                    (dict(ntr=2048), b"n_trainable"), (dict(ntr=0), b"n_trainable"), (dict(table=None, nr=1), b"bad args"),
                    (dict(table=C.c_void_p(0x2004)), b"8-byte aligned"),
                    # a null table with 0 ranges is the flat form, which keeps no EMA
                    (dict(table=None, nr=0, ema=p, ema_decay=0.9), b"keeps no EMA"),
                    (dict(table=None, nr=0, ema_decay=0.9), b"needs an ema buffer")):
        assert step(**kw) == 1, kw
        assert why in L.mrmt3_last_error(), (kw, L.mrmt3_last_error())
    ws = C.c_void_p(0x3000)
    need = L.mrmt3_grad_norm_workspace_elems()
    for args, why in (((p, 1022, tab, 1, 1.0, 0.0, 0, ws, need, p, p, None), b"multiple of 4"),
                      ((p, 1024, None, 1, 1.0, 0.0, 0, ws, need, p, p, None), b"null pointer"),
                      ((p, 1024, tab, 0, 1.0, 0.0, 0, ws, need, p, p, None), b"ranges"),
                      ((p, 1024, tab, -1, 1.0, 0.0, 0, ws, need, p, p, None), b"ranges"),
                      ((p, 1024, C.c_void_p(0x2004), 1, 1.0, 0.0, 0, ws, need, p, p, None), b"8-byte aligned"),
                      ((p, 1024, tab, 1, 1.0, -1.0, 0, ws, need, p, p, None), b"max_norm"),
                      ((p, 1024, tab, 1, 1.0, 0.0, 0, ws, 8, p, p, None), b"workspace")):
        assert L.mrmt3_grad_norm(*args) == 1, args
        assert why in L.mrmt3_last_error(), (args, L.mrmt3_last_error())


def test_binding_takes_weight_decay_from_the_table_only():
    """lib.adamw_step(ranges=...) with a weight_decay beside it is a ValueError before anything else is looked at."""
    from mrmt3 import lib
    t = lib.OptRanges([(0, 8, 0.01, 1.0)], 8)
    x = torch.zeros(8)
    with pytest.raises(ValueError, match="weight_decay comes from the range table"):
        lib.adamw_step(x, x, x, x, x[:1], torch.zeros(1, dtype=torch.int32), weight_decay=0.01, ranges=t)
    with pytest.raises(RuntimeError, match="device tensors"):                   # no CPU fallback, with or without a table
        lib.adamw_step(x, x, x, x, x[:1], torch.zeros(1, dtype=torch.int32), ranges=t)


# ---- checkpoint ------------------------------------------------------------------------------------------------------
def _cpu_trainer(model, groups, ema_decay, step=3):
    return SimpleNamespace(host_step=step, base_lr=1e-3, lr_lambda=None, lr_dev=torch.tensor([1e-3]), betas=(0.9, 0.999),
                           eps=1e-8, wd=0.01, groups=groups, ema_decay=ema_decay, accumulate=1)


def test_checkpoint_round_trip_of_ema_patterns_and_grouped_moments(tmp_path):
    from mrmt3 import checkpoint as ck
    from mrmt3.params import ParamGroups
    from models.t5 import T5ForConditionalGeneration
    m = T5ForConditionalGeneration(small_cfg())
    flat = m.flat
    gen = torch.Generator().manual_seed(1)
    flat.M, flat.V = torch.randn(flat.numel, generator=gen), torch.rand(flat.numel, generator=gen)
    flat.E = torch.randn(flat.numel, generator=gen)
    groups = ParamGroups(flat.shapes, frozen=["encoder.*"], no_decay=["*layer_norm.weight"], lr_scale={"lm_head.weight": 0.5})
    path = str(tmp_path / "g.ckpt")
    torch.save(ck.lightning_checkpoint(m, _cpu_trainer(m, groups, 0.99)), path)
    blob = ck.read_checkpoint(path)
    saved = blob["extra"]["groups"]
    assert saved == dict(frozen=["encoder.*"], no_decay=["*layer_norm.weight"], lr_scale={"lm_head.weight": 0.5}, ema_decay=0.99)
    assert list(blob["extra"]["ema"]) == list(flat.shapes)
    for k, v in blob["extra"]["ema"].items():
        assert torch.equal(v, flat.view(flat.E, k))
    # the moments come back into a second store: trainable tensors exactly, frozen ones untouched (they are not in the file)
    m2 = T5ForConditionalGeneration(small_cfg())
    f2 = m2.flat
    f2.M, f2.V = torch.full((f2.numel,), 7.0), torch.full((f2.numel,), 9.0)
    order = ck.reference_parameter_order(m.cfg, 0)
    g2 = ParamGroups(f2.shapes, saved["frozen"], saved["no_decay"], saved["lr_scale"])
    assert ck.adamw_state_to_flat(blob["optimizer"], f2, order, groups=g2, weight_decay=0.01) == 3
    for k in flat.shapes:
        if k in groups.frozen:
            assert bool((f2.view(f2.M, k) == 7.0).all()) and bool((f2.view(f2.V, k) == 9.0).all())
        else:
            assert torch.equal(f2.view(f2.M, k), flat.view(flat.M, k)) and torch.equal(f2.view(f2.V, k), flat.view(flat.V, k))
    with pytest.raises(ValueError, match="parameters"):
        ck.adamw_state_to_flat(blob["optimizer"], f2, order)                       # read as if nothing were frozen
    # a checkpoint written without any of the options has none of the new fields and reads as before
    torch.save(ck.lightning_checkpoint(m, _cpu_trainer(m, ParamGroups(flat.shapes), None)), path)
    blob = ck.read_checkpoint(path)
    assert "groups" not in blob["extra"] and "ema" not in blob["extra"]
    assert len(blob["optimizer"]["param_groups"]) == 1 and len(blob["optimizer"]["param_groups"][0]["params"]) == len(order)
    assert ck.adamw_state_to_flat(blob["optimizer"], f2, order) == 3
    assert torch.equal(f2.M, flat.M) and torch.equal(f2.V, flat.V)


def test_exported_optimizer_state_has_the_groups_torch_builds():
    """The same freeze and no-decay sets given to torch.optim.AdamW as real param groups: the exported state dict has the
    same groups (hyper-parameters, parameter ids), and torch loads it and finds each tensor's moments under its id."""
    from mrmt3 import checkpoint as ck
    from mrmt3.params import ParamGroups
    from models.t5 import T5ForConditionalGeneration
    m = T5ForConditionalGeneration(small_cfg())
    flat = m.flat
    gen = torch.Generator().manual_seed(2)
    flat.M, flat.V = torch.randn(flat.numel, generator=gen), torch.rand(flat.numel, generator=gen)
    frozen_p, nodecay_p = ["encoder.*"], ["*layer_norm.weight", "decoder_embed_tokens.weight"]
    groups = ParamGroups(flat.shapes, frozen=frozen_p, no_decay=nodecay_p)
    order = ck.reference_parameter_order(m.cfg, 0)
    got = ck.adamw_state_from_flat(flat, order, 5, 2e-4, (0.9, 0.999), 1e-8, 0.01, groups=groups)
    ref = TorchGroups({k: flat.master(k) for k in order}, order, frozen=match(order, frozen_p), no_decay=match(order, nodecay_p),
                      lr=2e-4, weight_decay=0.01)
    ref.step({k: torch.ones_like(flat.master(k)) for k in order})
    want = ref.opt.state_dict()
    # the first trainable parameter in model.parameters() order is the no-decay table here, so torch's [decay, no_decay]
    # construction order is the reverse of first appearance: compare the groups as a set keyed by weight decay
    assert len(got["param_groups"]) == len(want["param_groups"]) == 2
    by_wd = lambda sd: {g["weight_decay"]: g for g in sd["param_groups"]}
    trainable = [k for k in order if k not in groups.frozen]
    ids = [i for g in got["param_groups"] for i in g["params"]]
    assert ids == list(range(len(trainable))) and sorted(got["state"]) == ids            # frozen tensors: absent
    names = [k for _, _, ks in ck.optimizer_groups(order, groups, 0.01) for k in ks]
    for wd, g in by_wd(got).items():
        w = by_wd(want)[wd]
        assert len(g["params"]) == len(w["params"])
        for f in ("lr", "betas", "eps", "amsgrad", "maximize"):
            assert g[f] == w[f], f
        mine = [names[i] for i in g["params"]]
        theirs = [k for k in order if k not in groups.frozen and ((k in groups.no_decay) == (wd == 0.0))]
        assert mine == theirs
    # torch accepts it: an optimizer built over the same groups in the exported order loads the state
    params = {k: torch.nn.Parameter(flat.master(k).clone()) for k in order}
    opt = torch.optim.AdamW([dict(params=[params[names[i]] for i in g["params"]], weight_decay=g["weight_decay"])
                             for g in got["param_groups"]], lr=2e-4)
    opt.load_state_dict(got)
    for i, k in enumerate(names):
        assert torch.equal(opt.state[params[k]]["exp_avg"], flat.view(flat.M, k))
        assert torch.equal(opt.state[params[k]]["exp_avg_sq"], flat.view(flat.V, k))
    assert all(params[k] not in opt.state for k in groups.frozen)


# ---- train.py ---------------------------------------------------------------------------------------------------------
def test_train_py_reads_and_validates_the_group_keys():
    import train
    from mrmt3 import hydra_lite
    cfg = lambda **kw: hydra_lite._wrap({k: (hydra_lite._parse_value(v) if isinstance(v, str) else v) for k, v in kw.items()})
    assert train.group_options(cfg()) == (None, None, None, "train")
    got = train.group_options(cfg(freeze='["encoder.*", "proj.weight"]', no_decay='["*layer_norm.weight"]', ema_decay="0.999"))
    assert got == (["encoder.*", "proj.weight"], ["*layer_norm.weight"], 0.999, "train")
    assert train.group_options(cfg(ema_decay="0.9", export_weights="ema"))[2:] == (0.9, "ema")
    assert train.group_options(cfg(freeze="null", ema_decay="null")) == (None, None, None, "train")
    for kw, key in ((dict(freeze="encoder.*"), "freeze"), (dict(no_decay="[3]"), "no_decay"), (dict(no_decay="7"), "no_decay"),
                    (dict(ema_decay="1.0"), "ema_decay"), (dict(ema_decay="0"), "ema_decay"), (dict(ema_decay="abc"), "ema_decay"),
                    (dict(ema_decay="true"), "ema_decay"), (dict(export_weights="ema"), "ema_decay"),
                    (dict(export_weights="best"), "export_weights")):
        with pytest.raises(ValueError, match=key):
            train.group_options(cfg(**kw))
