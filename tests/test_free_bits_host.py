"""Host side of the KL controls: engine.kl_dims_reference / kl_dims_grad_reference against the independent numpy
restatement (tests/kl_ref.py) and torch autograd, the flags, check_kl_controls, the dispatch of loss_function and the
arithmetic of LatentReport.  No GPU."""
import argparse
import math

import numpy as np
import pytest
import torch

from gct_plus_amd import engine
from gct_plus_amd.Configuration.config import train_opts
from gct_plus_amd.Train import trainer1
from gct_plus_amd.Train.latent_report import LatentReport
from tests import kl_ref

BASE = ["-model_type", "vaetf", "-model_folder", "/nonexistent"]
SHAPES = [(1, 1, 4), (2, 3, 4), (5, 9, 128), (7, 37, 64), (4, 11, 12)]


def parse(extra):
    p = argparse.ArgumentParser()
    train_opts(p)
    return p.parse_args(BASE + extra)


def inputs(shape, mask):
    B, Le, D = shape
    mu, lv = kl_ref.latent_inputs(B, Le, D, seed=B * 1000 + Le * 10 + D)
    return mu, lv, kl_ref.live_masks(B, Le, seed=B + Le + D)[mask]


# ------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("mask", ["none", "random", "one_dead", "all_dead"])
@pytest.mark.parametrize("shape", SHAPES)
def test_engine_reference_matches_kl_ref(shape, mask):
    mu, lv, live = inputs(shape, mask)
    B, D = shape[0], shape[2]
    for lam in (0.0, 0.25, 0.05, 1e30):
        want = kl_ref.kl_dims(mu, lv, live, lam, B)
        got = engine.kl_dims_reference(torch.from_numpy(mu), torch.from_numpy(lv),
                                       None if live is None else torch.from_numpy(live), lam, B)
        # torch.exp and numpy.exp may differ by an ulp of fp32 per term: a part in 2^23 of e^l <= bound's scale
        tol = kl_ref.kl_dim_bound(mu, lv, live) / 8 + 1e-300
        assert np.all(np.abs(got["kl_dim"].numpy() - want["kl_dim"]) <= tol)
        assert got["floor"] == want["floor"] and got["live_rows"] == want["live_rows"]
        near = np.abs(want["kl_dim"] - want["floor"]) <= tol
        assert np.array_equal(got["gate"].numpy()[~near], want["gate"][~near])
        if not near.any():
            assert got["n_floor"] == want["n_floor"]
            assert abs(got["objective"] - want["objective"]) <= tol.sum() + 1e-15 * abs(want["objective"])
        assert abs(got["raw"] - want["raw"]) <= tol.sum()
        gm, gl = engine.kl_dims_grad_reference(torch.from_numpy(mu), torch.from_numpy(lv),
                                               None if live is None else torch.from_numpy(live), lam, B)
        wm, wl = kl_ref.kl_dims_grad(mu, lv, live, lam, B)
        if not near.any():
            assert np.allclose(gm.numpy(), wm, rtol=1e-14, atol=0) and np.allclose(gl.numpy(), wl, rtol=1e-13, atol=1e-16)


@pytest.mark.parametrize("shape", SHAPES)
def test_zero_floor_no_mask_is_the_plain_sum(shape):
    mu, lv, _ = inputs(shape, "none")
    got = engine.kl_dims_reference(mu, lv, None, 0.0, shape[0])
    m, l = mu.astype(np.float64), lv.astype(np.float64)
    plain = -0.5 * np.sum(1 + l - m * m - np.exp(l))
    assert got["gate"].all() and got["n_floor"] == 0 and got["objective"] == got["raw"]
    assert abs(got["raw"] - plain) <= kl_ref.kl_dim_bound(mu, lv).sum()
    gm, gl = engine.kl_dims_grad_reference(mu, lv, None, 0.0, shape[0])
    assert np.allclose(gm.numpy().reshape(shape), m, rtol=1e-15, atol=0)              # gct_kld_bwd's rule with g = 1
    assert np.allclose(gl.numpy().reshape(shape), 0.5 * (np.exp(l) - 1), rtol=1e-13, atol=1e-16)


@pytest.mark.parametrize("mask", ["none", "random"])
def test_reference_gradient_is_autograd_of_the_formula(mask):
    shape = (5, 9, 128)
    mu, lv, live = inputs(shape, mask)
    B, Le, D = shape
    m = torch.tensor(mu, dtype=torch.float64).view(-1, D).requires_grad_()
    l = torch.tensor(lv, dtype=torch.float64).view(-1, D).requires_grad_()
    keep = torch.ones(B * Le, dtype=torch.bool) if live is None else torch.from_numpy(live).view(-1)
    K = -0.5 * ((1 + l - m * m - l.exp()) * keep[:, None]).sum(0)
    floor = torch.tensor(0.25 * B, dtype=torch.float64)
    torch.maximum(K, floor).sum().backward()
    gm, gl = engine.kl_dims_grad_reference(mu, lv, live, 0.25, B)
    assert torch.allclose(gm, m.grad, rtol=1e-13, atol=0) and torch.allclose(gl, l.grad, rtol=1e-12, atol=1e-16)
    assert (gm[:, 0::2] == 0).all() and (gm[keep][:, 1::2] != 0).all()       # even dimensions sit on the floor


def test_objective_is_monotone_in_the_floor():
    mu, lv, live = inputs((7, 37, 64), "random")
    lams = [0.0, 0.01, 0.05, 0.25, 1.0, 4.0, 100.0]
    res = [engine.kl_dims_reference(mu, lv, live, lam, 7) for lam in lams]
    obj = [r["objective"] for r in res]
    assert all(a <= b for a, b in zip(obj, obj[1:])) and obj[0] < obj[-1]
    assert all(a["n_floor"] <= b["n_floor"] for a, b in zip(res, res[1:]))
    assert len({r["raw"] for r in res}) == 1 and all(r["objective"] >= r["raw"] for r in res)


def test_all_dead_mask():
    mu, lv, live = inputs((4, 11, 12), "all_dead")
    got = engine.kl_dims_reference(mu, lv, live, 0.25, 4)
    assert got["objective"] == 12 * 1.0 and got["raw"] == 0 and got["n_floor"] == 12 and got["live_rows"] == 0
    gm, gl = engine.kl_dims_grad_reference(mu, lv, live, 0.25, 4)
    assert (gm == 0).all() and (gl == 0).all()


# ------------------------------------------------------------------------------------------------------ the flags
def test_flags_default_to_off():
    a = parse([])
    assert a.kl_free_bits == 0.0 and a.kl_mask_pad is False and a.latent_report is False


def test_flags_parse():
    a = parse(["-kl_free_bits", "0.05", "-kl_mask_pad", "-latent_report"])
    assert a.kl_free_bits == 0.05 and a.kl_mask_pad is True and a.latent_report is True
    assert parse(["-kl_free_bits", "0"]).kl_free_bits == 0.0


@pytest.mark.parametrize("text", ["-1", "-0.5", "nan", "inf", "-inf", "1e39", "one", ""])
def test_kl_free_bits_rejects_negative_and_non_finite_values(text):
    with pytest.raises(SystemExit):
        parse(["-kl_free_bits", text])


def test_check_kl_controls():
    assert engine.check_kl_controls(0) == (0.0, False)
    assert engine.check_kl_controls(0.25, True) == (0.25, True)
    assert engine.check_kl_controls(2, 1) == (2.0, True)
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf"), 1e39, "0.1", None, True):
        with pytest.raises(ValueError):
            engine.check_kl_controls(bad)
    for bad in ("yes", 2, None, 0.5):
        with pytest.raises(ValueError):
            engine.check_kl_controls(0.1, bad)


# -------------------------------------------------------------------------------------------------- loss_function
class _Spy:
    def __init__(self, result):
        self.calls, self.result = [], result

    def apply(self, *a):
        self.calls.append(a)
        return self.result


def test_loss_function_dispatch(monkeypatch):
    """Default arguments: KldFn as before, KldFreeBitsFn never.  A floor or a mask: the other way round, the loss takes
    the objective and the returned KLD is the raw KL."""
    plain, fb, ce = _Spy(torch.tensor(3.0)), _Spy((torch.tensor(5.0), torch.tensor(2.0), None, None)), _Spy(torch.tensor(10.0))
    monkeypatch.setattr(engine, "KldFn", plain)
    monkeypatch.setattr(engine, "KldFreeBitsFn", fb)
    monkeypatch.setattr(engine, "CrossEntropySumFn", ce)
    mu = lv = torch.zeros(4, 6, 8)
    loss, rce, _, kld = trainer1.loss_function(0.5, None, "logits", None, "ys", mu, lv, False, 1)
    assert len(plain.calls) == 1 and plain.calls[0] == (mu, lv) and not fb.calls
    assert loss.item() == 11.5 and kld.item() == 3.0 and rce.item() == 10.0
    loss, _, _, kld = trainer1.loss_function(0.5, None, "logits", None, "ys", mu, lv, False, 1, free_bits=0.0,
                                             latent_live=None)
    assert len(plain.calls) == 2 and not fb.calls
    live = torch.ones(4, 1, 6, dtype=torch.bool)
    for kw in (dict(free_bits=0.25), dict(latent_live=live), dict(free_bits=0.25, latent_live=live)):
        n = len(fb.calls)
        loss, _, _, kld = trainer1.loss_function(0.5, None, "logits", None, "ys", mu, lv, False, 1, **kw)
        assert len(fb.calls) == n + 1 and len(plain.calls) == 2
        assert fb.calls[-1][2] is kw.get("latent_live") and fb.calls[-1][3] == kw.get("free_bits", 0.0)
        assert fb.calls[-1][4] == 4                                   # n_mol = the batch size
        assert loss.item() == 12.5 and kld.item() == 2.0              # RCE + beta * objective; KLD stays the raw KL
    with pytest.raises(TypeError):
        trainer1.loss_function(0.5, None, "logits", None, "ys", mu, lv, False, 1, 0.25)    # keyword-only


# --------------------------------------------------------------------------------------------------- LatentReport
def test_latent_report_arithmetic():
    D, rows, mols = 4, 10, 5
    mean = np.array([0.0, 0.5, -1.0, 0.2])
    var = np.array([0.0, 0.02, 0.25, 0.005])
    acc = np.zeros((6, D))
    acc[0] = rows * mean
    acc[1] = rows * (var + mean * mean)
    acc[2] = rows * np.array([1.0, 0.5, 0.3, 0.98])
    acc[3] = rows * np.log([1.0, 0.5, 0.3, 0.98])
    acc[4] = mols * np.array([0.0, 0.04, 2.0, 0.06])
    acc[5] = rows
    r = LatentReport.from_state(acc, mols, free_bits=0.05)
    assert np.allclose(r.mu_mean.numpy(), mean, atol=1e-15) and np.allclose(r.mu_var.numpy(), var, atol=1e-15)
    assert np.allclose(r.post_var.numpy(), [1.0, 0.5, 0.3, 0.98], atol=1e-15)
    assert np.allclose(r.kl.numpy(), [0.0, 0.04, 2.0, 0.06], atol=1e-15)
    assert r.active_units == 2 and r.under_floor == 2 and r.rows == rows and r.molecules == mols
    assert math.isclose(r.kl_per_molecule, 2.1, rel_tol=1e-14)
    assert LatentReport.from_state(acc, mols, threshold=0.1).active_units == 1
    line = r.line(3)
    assert "epoch 3" in line and "active units: 2/4" in line and "\n" not in line
    frame = r.to_frame()
    assert list(frame.columns) == ["KL", "MU_MEAN", "MU_VAR", "POST_VAR", "ACTIVE"] and len(frame) == D
    assert frame["ACTIVE"].tolist() == [0, 1, 1, 0]
    empty = LatentReport.from_state(np.zeros((6, D)), 0)                 # nothing seen: zeros, not NaN
    assert empty.active_units == 0 and empty.kl_per_molecule == 0.0 and not torch.isnan(empty.mu_var).any()
    with pytest.raises(ValueError):
        LatentReport.from_state(np.zeros((5, D)), 1)
