"""The KL controls through the model and the trainer on the GPU: free bits and the pad mask in loss_function on a tiny
pvaetf (N 2, d_model 64, latent 16, dropout 0), and a train1 run with -kl_free_bits -kl_mask_pad -latent_report."""
import logging
import os

import pandas as pd
import pytest
import torch

from gct_plus_amd import synthetic

pytestmark = pytest.mark.gpu
PAD = synthetic.PAD_ID
MTYPE = "pvaetf"


@pytest.fixture(scope="module")
def rig():
    from gct_plus_amd.Model import model_dict
    vs, vt = synthetic.vocab_sizes(MTYPE)
    torch.manual_seed(1)
    model = model_dict[MTYPE](vs, vt, dropout=0.0, nconds=synthetic.n_conds(MTYPE), use_cond2dec=False,
                              use_cond2lat=True, N=2, d_model=64, dff=128, h=4, latent_dim=16).cuda().train()
    batch = {k: v.cuda() for k, v in synthetic.make_dataset(6, max_len=48, model_type=MTYPE, seed=99).items()}
    torch.manual_seed(2)
    sampler = model.sampler if hasattr(model, "sampler") else model.encoder
    sampler.eps_override = torch.randn(6, 48 + synthetic.n_conds(MTYPE), 16)            # the same z in every forward
    return model, batch


def step(model, batch, **kl):
    """One forward and loss_function(**kl); returns (loss, RCE, KLD, mu) with mu's gradient retained."""
    from gct_plus_amd.Model import forward_propagation
    from gct_plus_amd.Train.trainer1 import loss_function
    model.zero_grad(set_to_none=True)
    prop, mol, mu, lv, _ = forward_propagation[MTYPE](model, batch, PAD, False)[:5]
    mu.retain_grad()
    nc = synthetic.n_conds(MTYPE)
    ys_cond = batch["dconds"].unsqueeze(2).contiguous().view(-1, nc, 1)
    loss, rce, _, kld = loss_function(0.04, prop, mol, ys_cond, batch["trg"][:, 1:].contiguous().view(-1), mu, lv,
                                      False, PAD, **kl)
    return loss, rce, kld, mu


def grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def test_huge_floor_leaves_the_reconstruction_gradient(rig):
    """Every dimension on the floor: the KL term is a constant, so the parameter gradients are those of RCE alone,
    bit for bit (a zero may change its sign: g + 0.0)."""
    model, batch = rig
    loss, rce, kld, _ = step(model, batch, free_bits=1e30)
    loss.backward()
    with_floor = grads(model)
    assert torch.isfinite(loss) and loss.item() > 1e29 and 0 < kld.item() < 1e6         # KLD stays the raw KL
    loss2, rce2, _, _ = step(model, batch)
    rce2.backward()
    rce_only = grads(model)
    assert torch.equal(rce, rce2)
    assert with_floor.keys() == rce_only.keys() and len(rce_only) > 10
    for name in rce_only:
        assert torch.equal(with_floor[name], rce_only[name]), name            # (-0.0 == 0.0 under torch.equal)


def test_pad_mask_zeroes_the_kl_gradient_of_padded_rows(rig):
    from gct_plus_amd.Model.forward_propagation1 import latent_live_rows
    model, batch = rig
    live = latent_live_rows(MTYPE, batch, PAD)
    nc = synthetic.n_conds(MTYPE)
    assert live.shape == (6, 1, 48 + nc) and live[:, 0, :nc].all()                 # condition rows always count
    assert torch.equal(live[:, 0, nc:], batch["src"] != PAD) and not live.all() and live[0].all()
    loss, _, kld, mu = step(model, batch)
    loss.backward()
    plain = mu.grad.clone()                                                          # the KL path's gradient: beta * mu
    loss_m, _, kld_m, mu_m = step(model, batch, latent_live=live)
    loss_m.backward()
    masked = mu_m.grad
    keep = live[:, 0, :]
    assert (plain[~keep] != 0).any()
    assert (masked[~keep] == 0).all() and torch.equal(masked[keep], plain[keep])
    assert 0 < kld_m.item() < kld.item() and loss_m.item() < loss.item()


def test_train1_with_kl_controls_and_latent_report(tmp_path, caplog):
    from gct_plus_amd import train1
    from gct_plus_amd.Model import model_dict
    from gct_plus_amd.Model.forward_propagation1 import latent_live_rows
    folder = str(tmp_path / "exp")
    flags = ("-seed 1 -use_cond2lat -model_type pvaetf -property_list logP tPSA QED -N 2 -d_model 64 -d_ff 128 "
             f"-H 4 -latent_dim 16 -batch_size 16 -model_folder {folder} -synthetic 64 -synthetic_valid 32 "
             "-max_strlen 48 -print_every 100 -kl_free_bits 0.05 -kl_mask_pad -latent_report -num_epoch 1").split()
    log = logging.getLogger("train")
    before = list(log.handlers)
    try:
        with caplog.at_level(logging.INFO, logger="train"):
            train1.main(0, 1, flags)
    finally:
        # train1.get_logger binds the process-wide "train" logger to the first run's records.log and keeps it: hand
        # the logger back as it was, so that a later run in this process opens its own file
        for h in [h for h in log.handlers if h not in before]:
            log.removeHandler(h)
            h.close()
    t1 = pd.read_csv(os.path.join(folder, "train_1.csv"), index_col=0)
    assert list(t1.columns) == ["RCE", "KLD", "LOSS", "BETA", "LR"] and len(t1) == 4
    assert t1.notna().all().all() and (t1["KLD"] > 0).all()
    # LOSS is what was optimised: RCE + beta * objective, and the objective is never below the raw KL
    assert (t1["LOSS"] >= t1["RCE"] + t1["BETA"] * t1["KLD"] - 1e-4 * t1["LOSS"].abs()).all()
    lat = pd.read_csv(os.path.join(folder, "latent_1.csv"), index_col=0)
    assert len(lat) == 16 and list(lat.columns) == ["KL", "MU_MEAN", "MU_VAR", "POST_VAR", "ACTIVE"]
    assert lat.notna().all().all() and (lat["POST_VAR"] > 0).all() and (lat["KL"] >= 0).all()
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("LATENT")]
    assert len(lines) == 1 and "epoch 1" in lines[0]
    active = int(lines[0].split("active units: ")[1].split("/")[0])
    assert active == int(lat["ACTIVE"].sum())

    # the same count from model.encode on the host: the checkpoint is the model the report saw
    ck = torch.load(os.path.join(folder, "model_1.pt"), map_location="cpu", weights_only=True)
    vs, vt = synthetic.vocab_sizes(MTYPE)
    model = model_dict[MTYPE](vs, vt, dropout=0.1, nconds=3, use_cond2dec=False, use_cond2lat=True, N=2, d_model=64,
                              dff=128, h=4, latent_dim=16)
    model.load_state_dict(ck["model_state_dict"])
    model = model.cuda().eval()
    valid = {k: v.cuda() for k, v in synthetic.make_dataset(32, 48, MTYPE, seed=1).items()}
    rows = []
    with torch.no_grad():
        for b in synthetic.batches(valid, 16):
            live = latent_live_rows(MTYPE, b, PAD)
            mu = model.encode(b["src"], live, b["econds"])[1]
            rows.append(mu[live[:, 0, :]].double().cpu())
    var = torch.cat(rows).var(dim=0, unbiased=False)
    assert not ((var - 0.01).abs() < 1e-6).any(), "a dimension sits on the threshold: the count is not well defined"
    assert int((var > 0.01).sum()) == active
    assert torch.allclose(torch.tensor(lat["MU_VAR"].values), var, rtol=1e-9, atol=1e-12)
