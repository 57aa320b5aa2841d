"""Gradient clipping without a GPU: train.py's reading of `trainer.gradient_clip_val` / `trainer.gradient_clip_algorithm`
on composed configs, the trainer's argument validation, and the norm / step entry points in the header and the binding."""
import ctypes

import pytest

from mrmt3 import hydra_lite, lib
from test_config_cpu import MODEL, TOP


@pytest.fixture()
def cfgdir(tmp_path):
    (tmp_path / "model").mkdir()
    (tmp_path / "dataset").mkdir()
    (tmp_path / "config.yaml").write_text(TOP)
    (tmp_path / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    return str(tmp_path)


def test_gradient_clipping_reads_the_trainer_block(cfgdir):
    import train
    assert train.gradient_clipping(hydra_lite.compose(cfgdir, "config", [])) == (None, "norm")
    assert train.gradient_clipping(hydra_lite.compose(cfgdir, "config", ["+trainer.gradient_clip_val=0.5"])) == (0.5, "norm")
    cfg = hydra_lite.compose(cfgdir, "config", ["+trainer.gradient_clip_val=2", "+trainer.gradient_clip_algorithm=value"])
    assert train.gradient_clipping(cfg) == (2.0, "value")
    # Lightning: 0 (and null) mean "no clipping"
    assert train.gradient_clipping(hydra_lite.compose(cfgdir, "config", ["+trainer.gradient_clip_val=0"])) == (None, "norm")
    assert train.gradient_clipping(hydra_lite.compose(cfgdir, "config", ["+trainer.gradient_clip_val=null"])) == (None, "norm")
    cfg = hydra_lite.compose(cfgdir, "config", ["+trainer.gradient_clip_val=1.0", "+trainer.gradient_clip_algorithm=agc"])
    with pytest.raises(ValueError, match="agc"):
        train.gradient_clipping(cfg)
    # a config without a trainer block at all
    assert train.gradient_clipping({}) == (None, "norm")


def test_clip_options_validation():
    from mrmt3.trainer import clip_options
    assert clip_options() == (False, 0.0, 0.0, False)
    assert clip_options(0.5) == (True, 0.5, 0.0, False)
    assert clip_options(0.5, "value") == (True, 0.0, 0.5, False)
    assert clip_options(2, None) == (True, 2.0, 0.0, False)
    assert clip_options(skip_nonfinite=True) == (True, 0.0, 0.0, True)
    assert clip_options(track_grad_norm=True) == (True, 0.0, 0.0, False)
    assert clip_options(None, "value") == (False, 0.0, 0.0, False)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "1.0", True):
        with pytest.raises(ValueError, match="gradient_clip_val"):
            clip_options(bad)
    with pytest.raises(ValueError, match="'agc'"):
        clip_options(1.0, "agc")
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        clip_options(None, "Norm")


def test_new_entry_points_are_declared_bound_and_exported():
    vp, ci, cf, csz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    want = {
        "mrmt3_grad_norm_workspace_elems": (csz, []),
        "mrmt3_grad_norm": (ci, [vp, csz, vp, ci, cf, cf, ci, vp, csz, vp, vp, vp]),
        "mrmt3_adamw_step": (ci, [vp, vp, vp, vp, vp, csz, vp, ci, csz, vp, vp, cf, cf, cf, cf, cf, cf, vp, cf, vp, vp]),
    }
    names = lib.header_symbols()
    for name, sig in want.items():
        assert name in names and lib._SIGS[name] == sig, (name, lib._SIGS.get(name))
    # one step and one norm: the header declares no sibling of either
    assert {n for n in names if "adamw" in n or "grad_norm" in n} == set(want)
    so = lib.load()
    assert so.mrmt3_version() >= 121 and lib.MIN_VERSION >= 121
    assert so.mrmt3_grad_norm_workspace_elems() >= 2 and so.mrmt3_grad_norm_workspace_elems() % 2 == 0
    assert callable(lib.grad_norm) and callable(lib.adamw_step)
    assert "grad_norm" not in lib.COUNTER_NAMES and len(lib.COUNTER_NAMES) == 19      # 17 families + the two log-mel kernels
    # argument errors come back as codes with a message, before anything is launched (no device needed)
    buf = (ctypes.c_double * 8)()
    a = (ctypes.addressof(buf) + 15) & ~15
    assert so.mrmt3_grad_norm(a, 6, None, 0, 1.0, 0.0, 0, a, 1 << 20, a, a, None) != 0 and b"multiple of 4" in so.mrmt3_last_error()
    assert so.mrmt3_grad_norm(a, 8, None, 0, 1.0, 0.0, 0, a, 16, a, a, None) != 0 and b"workspace" in so.mrmt3_last_error()
    assert so.mrmt3_grad_norm(a, 8, None, 0, 1.0, -1.0, 0, a, 1 << 20, a, a, None) != 0 and b"max_norm" in so.mrmt3_last_error()
    assert so.mrmt3_grad_norm(None, 8, None, 0, 1.0, 0.0, 0, a, 1 << 20, a, a, None) != 0 and b"null" in so.mrmt3_last_error()

    def flat_step(stat, clip, n=8, p=a):       # the flat form: no ema, no table
        return so.mrmt3_adamw_step(p, a, a, a, None, n, None, 0, 0, a, a, 0.9, 0.999, 1e-8, 0.01, 1.0, 0.0, stat, clip, None, None)
    assert flat_step(None, 0.5) != 0 and b"needs stat_dev" in so.mrmt3_last_error()      # a clamp without the clipped form
    assert flat_step(a, -1.0) != 0 and b"clip_value" in so.mrmt3_last_error()
    assert flat_step(None, -1.0) != 0 and b"clip_value" in so.mrmt3_last_error()
    assert flat_step(a, 0.0, n=6) != 0 and b"bad args" in so.mrmt3_last_error()
    assert flat_step(a, 0.0, p=None) != 0 and b"bad args" in so.mrmt3_last_error()
