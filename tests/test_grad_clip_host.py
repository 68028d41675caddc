"""CPU: the host side of global gradient-norm clipping -- the train1 flag (-max_grad_norm, default 0 = off), FusedAdam's
and the fine-tuning functions' argument validation, the torch.nn.utils.clip_grad_norm_ leg of the fine-tuning functions
for optimizers that are not FusedAdam, the ABI number, and clip_reference, the fp64 rule the GPU tests compare with."""
import argparse
import math
import os
import re

import pytest
import torch

from gct_plus_amd import _lib
from gct_plus_amd.Configuration.config import train_opts

BASE = ["-model_type", "vaetf", "-model_folder", "/nonexistent"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 8 words of the device state (include/gctplus_hip.h: gct_grad_norm)
NORM, COEF, NONFINITE, STEPS, CLIPPED_STEPS, NONFINITE_STEPS, LARGEST, RESERVED = range(8)


def clip_reference(g, gscale, max_norm):
    """The rule in fp64 on the float32 values of the two host scalars: (norm, coef, nonfinite) with
    norm = |gscale| * sqrt(sum g^2), coef = min(1, max_norm / (norm + 1e-6)); nonfinite when norm, rounded to fp32, is
    inf or NaN (coef is then 0: the step is skipped)."""
    gscale = float(torch.tensor(gscale, dtype=torch.float32))
    max_norm = float(torch.tensor(max_norm, dtype=torch.float32))
    norm = abs(gscale) * math.sqrt(float(g.detach().cpu().double().pow(2).sum())) if g.numel() else 0.0
    if not bool(torch.isfinite(torch.tensor(norm, dtype=torch.float64).float())):
        return norm, 0.0, True
    return norm, min(1.0, max_norm / (norm + 1e-6)), False


def parse(extra):
    p = argparse.ArgumentParser()
    train_opts(p)
    return p.parse_args(BASE + extra)


# --------------------------------------------------------------------------------------------------------- the flag
def test_max_grad_norm_defaults_to_off():
    assert parse([]).max_grad_norm == 0.0


@pytest.mark.parametrize("text,value", [("1.0", 1.0), ("0.5", 0.5), ("0", 0.0), ("1e3", 1000.0)])
def test_max_grad_norm_accepts_a_float(text, value):
    got = parse(["-max_grad_norm", text]).max_grad_norm
    assert isinstance(got, float) and got == value


@pytest.mark.parametrize("text", ["-1", "-0.5", "nan", "inf", "-inf", "one", ""])
def test_max_grad_norm_rejects_negative_and_non_finite_values(text):
    with pytest.raises(SystemExit):
        parse(["-max_grad_norm", text])


# ------------------------------------------------------------------------------------------------------- FusedAdam
def _params():
    return [torch.nn.Parameter(torch.zeros(3))]


def test_fused_adam_takes_max_grad_norm_and_keeps_the_checkpoint_layout():
    from gct_plus_amd.optim import FusedAdam
    off, on = FusedAdam(_params()), FusedAdam(_params(), max_grad_norm=2)
    assert off.max_grad_norm is None and on.max_grad_norm == 2.0 and on.clip_state is None
    assert off.state_dict() == on.state_dict()                     # the setting is not part of the checkpoint
    assert set(on.state_dict()["param_groups"][0]) == set(torch.optim.Adam(_params()).state_dict()["param_groups"][0])
    assert on.grad_norm_stats() == dict(norm=0.0, coef=1.0, steps=0, clipped_steps=0, nonfinite_steps=0, max_norm=0.0)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), "1.0", True, 1e39, [1.0]])
def test_fused_adam_refuses_a_bad_max_grad_norm(bad):
    from gct_plus_amd.optim import FusedAdam
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam(_params(), max_grad_norm=bad)
    opt = FusedAdam(_params())
    opt.max_grad_norm = bad                                         # a settable attribute: refused at step(), before
    with pytest.raises(ValueError, match="max_grad_norm"):          # any device work (the parameter is a CPU tensor
        opt.step()                                                  # without a gradient: nothing else could raise this)


# ------------------------------------------------------------------------------------------- the fine-tuning functions
class Untouched:                                                    # any use of the sampler would raise
    model = None


@pytest.mark.parametrize("bad", [0, -1.0, float("nan"), float("inf"), "1.0"])
def test_fine_tuning_refuses_a_bad_max_grad_norm_before_device_work(bad):
    from gct_plus_amd.Train.finetune import ppo_update, reinforce_step
    rows = (None, torch.zeros(3, 5, dtype=torch.long))
    with pytest.raises(ValueError, match="max_grad_norm"):
        reinforce_step(Untouched(), None, rows, torch.zeros(3), max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        ppo_update(Untouched(), None, rows, torch.zeros(3), max_grad_norm=bad)


def test_a_stock_optimizer_is_clipped_with_clip_grad_norm_between_backward_and_step():
    """The leg of reinforce_step / ppo_update for optimizers that are not FusedAdam, on a CPU parameter: SGD with lr 1
    makes the applied gradient visible as the parameter's change."""
    from gct_plus_amd.Train.finetune import _GradClip
    g = torch.tensor([3.0, 4.0, 12.0])                              # norm 13
    for max_norm, clipped in ((6.5, True), (26.0, False)):
        p = torch.nn.Parameter(torch.zeros(3))
        opt = torch.optim.SGD([p], lr=1.0)
        clip = _GradClip(opt, max_norm, "test")
        assert clip.active and not clip.fused
        clip.install()
        p.grad = g.clone()
        clip.step()
        clip.restore()
        norm, coef, _ = clip_reference(g, 1.0, max_norm)
        got_norm, got_clipped = clip.norm_and_clipped()
        assert abs(float(got_norm) - norm) <= 2.0 ** -22 * norm and bool(got_clipped) == clipped == (coef < 1)
        assert torch.allclose(-p.detach(), g * coef, rtol=1e-6, atol=0)
    off = _GradClip(torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=1.0), None, "test")
    assert not off.active


def test_the_call_value_is_installed_on_a_fused_adam_and_put_back():
    from gct_plus_amd.optim import FusedAdam
    from gct_plus_amd.Train.finetune import _GradClip
    opt = FusedAdam(_params(), max_grad_norm=5.0)
    own = _GradClip(opt, None, "test")                              # None: the optimizer's own setting applies
    assert own.active and own.value == 5.0
    call = _GradClip(opt, 0.25, "test")
    call.install()
    assert opt.max_grad_norm == 0.25
    call.restore()
    assert opt.max_grad_norm == 5.0
    assert not _GradClip(FusedAdam(_params()), None, "test").active


# ------------------------------------------------------------------------------------------------- clip_reference, ABI
def test_clip_reference():
    g = torch.tensor([3.0, -4.0])
    assert clip_reference(g, 1.0, 10.0) == (5.0, 1.0, False)
    norm, coef, bad = clip_reference(g, 0.5, 1.0)
    assert norm == 2.5 and coef == 1.0 / (2.5 + 1e-6) and not bad
    assert clip_reference(torch.zeros(0), 1.0, 1.0) == (0.0, 1.0, False)
    assert clip_reference(torch.tensor([1.0, float("inf")]), 1.0, 1.0)[1:] == (0.0, True)
    assert clip_reference(torch.tensor([float("nan")]), 1.0, 1.0)[1:] == (0.0, True)
    assert clip_reference(torch.full((4,), 3e38), 1.0, 1.0)[1:] == (0.0, True)      # 6e38 is beyond fp32


def test_abi_version_is_33_in_the_header_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "gctplus_hip.h")).read()
    assert int(re.search(r"^#define GCT_ABI_VERSION (\d+)$", hdr, flags=re.M).group(1)) == _lib.ABI_VERSION == 33
    for name in ("gct_grad_norm", "gct_grad_norm_ws_bytes", "gct_adam_step"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gct_adam_step"][1]) == 14            # the nullable clip_state in front of the stream
    assert len(_lib.SIGNATURES["gct_grad_norm"][1]) == 7
