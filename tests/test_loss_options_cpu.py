"""Label smoothing and z-loss without a GPU: the float64 closed forms of tests/loss_ref.py (what the GPU tests compare the
kernels against) pinned to torch's own cross_entropy and to autograd, the argument validation of the binding, the trainer
and the C ABI, the two new entry points in the header and the library, and train.py's reading of the two keys and its step
line."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import loss_ref
from mrmt3 import hydra_lite, lib
from test_config_cpu import MODEL, TOP


# ---- 1. the closed forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_objective_without_z_is_torch_label_smoothing(eps):
    """z = 0, no weighting: the objective is F.cross_entropy(label_smoothing=eps, ignore_index=-100), mean reduction, in
    float64 (both sides are sums of about 30 terms of size 10: 1e-12 is a few hundred ulp of slack), and the second scalar
    is the plain cross-entropy whatever eps is."""
    logits, targets = loss_ref.case(37, 1536, weighted=False)
    l = logits.double()
    obj, nll = loss_ref.objective(l, targets, eps=eps)
    want = F.cross_entropy(l, targets, ignore_index=-100, label_smoothing=eps)
    assert abs(float(obj) - float(want)) < 1e-12 * abs(float(want))
    assert abs(float(nll) - float(F.cross_entropy(l, targets, ignore_index=-100))) < 1e-12 * abs(float(nll))
    if eps == 0.0:
        assert float(obj) == float(nll)


def test_z_term_is_t5x_z_loss():
    """objective(eps = 0, z) - nll = z * sum over scored rows of logsumexp^2 / number of scored rows."""
    logits, targets = loss_ref.case(37, 1100, weighted=False)
    l = logits.double()
    obj, nll = loss_ref.objective(l, targets, z=1e-4)
    scored = targets != -100
    want = 1e-4 * (torch.logsumexp(l, -1)[scored] ** 2).sum() / scored.sum()
    assert abs(float(obj - nll) - float(want)) < 1e-12
    assert float(want) > 1e-3            # (the +80 row alone gives 1e-4 * 87^2 / 29)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps,z", [(0.1, 0.0), (0.0, 1e-4), (0.1, 1e-4)])
def test_closed_form_gradient_is_autograd(eps, z, weighted):
    """float64: the gradient formula against autograd of the objective; ignored rows are exactly zero; every scored row of
    the gradient sums to grad_scale * w/denom * 2 z lse (softmax sums to 1, the two target terms to -1)."""
    logits, targets = loss_ref.case(37, 1536, weighted=weighted)
    l = logits.double().requires_grad_(True)
    obj, _ = loss_ref.objective(l, targets, eps=eps, z=z, weighted=weighted)
    obj.backward()
    g = loss_ref.gradient(logits, targets, eps=eps, z=z, weighted=weighted)
    assert float((g - l.grad).abs().max()) < 1e-15
    assert float(g[targets == -100].abs().max()) == 0.0
    g3 = loss_ref.gradient(logits, targets, eps=eps, z=z, weighted=weighted, grad_scale=3.0)
    assert torch.allclose(g3, 3.0 * g, rtol=1e-15, atol=0)
    w, n = loss_ref.weights(targets, weighted)
    if weighted:
        assert set(w.tolist()) == {0.0, 1.0, 3.0} and float(n.sum()) > float((targets != -100).sum())
    rowsum = w / n.sum() * 2.0 * z * torch.logsumexp(logits.double(), -1)
    assert float((g.sum(-1) - rowsum).abs().max()) < 1e-15


def test_weighted_objective_multiplies_the_whole_row_term():
    logits, targets = loss_ref.case(37, 1536, weighted=True)
    l = logits.double()
    obj, nll = loss_ref.objective(l, targets, eps=0.1, z=1e-4, weighted=True)
    w, n = loss_ref.weights(targets, True)
    lse = torch.logsumexp(l, -1)
    rows = torch.nonzero(targets != -100)[:, 0]
    r = torch.zeros(37, dtype=torch.float64)
    for i in rows.tolist():
        r[i] = 0.9 * (lse[i] - l[i, targets[i]]) + 0.1 * (lse[i] - l[i].mean()) + 1e-4 * lse[i] ** 2
    assert abs(float(obj) - float((w * r).sum() / n.sum())) < 1e-12
    lo, hi = loss_ref.inst_range(1536)
    assert (lo, hi) == (1135, 1262) and bool(((targets >= lo) & (targets <= hi)).any())


# ---- 2. validation ---------------------------------------------------------------------------------------------------
def test_ce_options_validation():
    assert lib.ce_options() == (False, 0.0, 0.0)
    assert lib.ce_options(0, 0) == (False, 0.0, 0.0)
    assert lib.ce_options(0.1) == (True, 0.1, 0.0)
    assert lib.ce_options(z_loss=1e-4) == (True, 0.0, 1e-4)
    for bad in (1, 1.0, 1.5, -0.1, float("nan"), "0.1", None, True):
        with pytest.raises(ValueError, match="label_smoothing"):
            lib.ce_options(bad, 0.0)
    for bad in (-1e-4, float("nan"), float("inf"), "1e-4", None, False):
        with pytest.raises(ValueError, match="z_loss"):
            lib.ce_options(0.0, bad)


def test_new_entry_points_are_declared_bound_and_validate_before_any_launch():
    vp, ci, cf, csz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    want = {
        "mrmt3_ce_fwd_bwd_reg": (ci, [vp, vp, vp, cf, cf, vp, vp, ci, ci, ci, ci, ci, ci, cf, vp]),
        "mrmt3_lmhead_ce_fwd_bwd_reg": (ci, [vp, ci, vp, ci, vp, vp, cf, cf, vp, vp, ci, ci, ci, ci, ci, ci, ci, cf, vp, csz, ci, vp]),
    }
    names = lib.header_symbols()
    for name, sig in want.items():
        assert name in names and lib._SIGS[name] == sig, (name, lib._SIGS.get(name))
    # the new entry points = the old ones' arguments with (label_smoothing, z_loss) in front of loss_dev
    for new, old in (("mrmt3_ce_fwd_bwd_reg", "mrmt3_ce_fwd_bwd"), ("mrmt3_lmhead_ce_fwd_bwd_reg", "mrmt3_lmhead_ce_fwd_bwd")):
        at = 3 if old == "mrmt3_ce_fwd_bwd" else 6
        plain = lib._SIGS[old][1]
        assert want[new][1] == plain[:at] + [cf, cf] + plain[at:]
    so = lib.load()
    assert so.mrmt3_version() >= 118 and lib.MIN_VERSION >= 118
    # no new dispatch counter for the loss: an untouched step counts as before (17 families + the two log-mel kernels)
    assert len(lib.COUNTER_NAMES) == 19 and not any("ce" in n.split("_") or "loss" in n for n in lib.COUNTER_NAMES)
    buf = (ctypes.c_double * 8)()
    a = (ctypes.addressof(buf) + 15) & ~15
    for eps, z, word in ((1.0, 0.0, b"label_smoothing"), (-0.1, 0.0, b"label_smoothing"), (float("nan"), 0.0, b"label_smoothing"),
                         (0.1, -1e-4, b"z_loss"), (0.1, float("nan"), b"z_loss"), (0.1, float("inf"), b"z_loss")):
        assert so.mrmt3_ce_fwd_bwd_reg(a, a, a, eps, z, a, None, 0, 4, 1536, 0, 0, 0, 1.0, None) == 1       # MRMT3_ERR_INVALID_ARG
        assert word in so.mrmt3_last_error(), (eps, z, so.mrmt3_last_error())
        assert so.mrmt3_lmhead_ce_fwd_bwd_reg(a, 512, a, 512, a, a, eps, z, a, None, 0, 4, 1536, 512, 0, 0, 0, 1.0, a, 1 << 20,
                                              1024, None) == 1
        assert word in so.mrmt3_last_error(), (eps, z, so.mrmt3_last_error())
    assert so.mrmt3_ce_fwd_bwd_reg(None, a, a, 0.1, 1e-4, a, None, 0, 4, 1536, 0, 0, 0, 1.0, None) == 1
    assert so.mrmt3_ce_fwd_bwd_reg(a, a, a, 0.1, 1e-4, a, None, 0, 4, 1538, 0, 0, 0, 1.0, None) == 1       # V % 4 != 0
    assert so.mrmt3_lmhead_ce_fwd_bwd_reg(a, 512, a, 512, a, a, 0.1, 1e-4, a, None, 0, 4, 1536, 512, 0, 0, 0, 1.0, a, 64, 1024,
                                          None) == 1
    assert b"workspace" in so.mrmt3_last_error()


def test_wrappers_and_trainer_refuse_bad_options_before_touching_the_device():
    """ValueError from the host-side check: it comes before the first device call, so CPU tensors get that far."""
    from mrmt3.trainer import Trainer
    logits, targets = torch.zeros(4, 1536), torch.zeros(4, dtype=torch.int64)
    for kw in ({"label_smoothing": 1.0}, {"label_smoothing": -0.5}, {"z_loss": -1.0}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            lib.cross_entropy(logits, targets, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            lib.lmhead_cross_entropy(logits.bfloat16(), logits.bfloat16(), targets, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            Trainer(None, **kw)


# ---- 3. train.py -----------------------------------------------------------------------------------------------------
@pytest.fixture()
def cfgdir(tmp_path):
    (tmp_path / "model").mkdir()
    (tmp_path / "dataset").mkdir()
    (tmp_path / "config.yaml").write_text(TOP)
    (tmp_path / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    return str(tmp_path)


def test_train_py_reads_the_two_keys(cfgdir):
    import train
    assert train.loss_options(hydra_lite.compose(cfgdir, "config", [])) == (0.0, 0.0)
    assert train.loss_options(hydra_lite.compose(cfgdir, "config", ["+label_smoothing=0.1", "+z_loss=1e-4"])) == (0.1, 1e-4)
    assert train.loss_options(hydra_lite.compose(cfgdir, "config", ["+z_loss=0.0001"])) == (0.0, 1e-4)
    assert train.loss_options(hydra_lite.compose(cfgdir, "config", ["+label_smoothing=null", "+z_loss=0"])) == (0.0, 0.0)
    assert train.loss_options({}) == (0.0, 0.0)
    assert train.loss_options({"label_smoothing": "0.2"}) == (0.2, 0.0)
    with pytest.raises(ValueError, match="label_smoothing"):
        train.loss_options(hydra_lite.compose(cfgdir, "config", ["+label_smoothing=1"]))
    with pytest.raises(ValueError, match="z_loss"):
        train.loss_options(hydra_lite.compose(cfgdir, "config", ["+z_loss=-1e-4"]))
    with pytest.raises(ValueError, match="label_smoothing"):
        train.loss_options({"label_smoothing": "lots"})


def test_step_line_format():
    import train
    assert train.format_step_line(7, 2.5) == "step 7 train_loss 2.5000"                      # both off: the line of before
    assert train.format_step_line(7, 2.5, grad_norm=0.125) == "step 7 train_loss 2.5000 grad_norm 0.1250"
    assert train.format_step_line(7, 2.75, nll=2.5) == "step 7 train_loss 2.7500 nll 2.5000"
    assert train.format_step_line(7, 2.75, nll=2.5, grad_norm=3) == "step 7 train_loss 2.7500 nll 2.5000 grad_norm 3.0000"
