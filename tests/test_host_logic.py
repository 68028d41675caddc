"""CPU-only tests of the host side: C-ABI symbol table, flag surface, schedules, data sharding,
mask builders, init-order parity of the product modules, flat-buffer bookkeeping."""
import argparse
import ctypes
import os
import re

import pytest
import torch

from gct_plus_amd import _lib, synthetic
from oracle import gct_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    """include/gctplus_hip.h <-> _lib.SIGNATURES <-> the built .so (no compute call)."""
    hdr = open(os.path.join(ROOT, "include", "gctplus_hip.h")).read()
    declared = set(re.findall(r"\b(gct_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.gct_version() == _lib.ABI_VERSION
    assert lib.gct_wgrad_ws_bytes(40960, 512, 512) > 0
    # the diagnostics library has its own header and is NOT part of the operator ABI
    dh = open(os.path.join(ROOT, "include", "gctplus_diag.h")).read()
    ddecl = set(re.findall(r"\b(gct_[a-z0-9_]+)\s*\(", dh))
    assert ddecl == set(_lib.DIAG_SIGNATURES) and not (ddecl & declared), (ddecl, declared & ddecl)
    dl = _lib.load_diag()
    for name in ddecl:
        assert hasattr(dl, name), name


def test_attention_direct_key_limit_has_one_owner():
    """GCT_ATTN_DIRECT_MAX_KEYS (header) is ops.ATTN_DIRECT_MAX_KEYS, and the direct backward's workspace exists up to
    it only: positive at the limit (per padded query row a 16-B record and limit / 32 keep words, per query tile one
    word rounded up to 16 B), 0 one key above it (the LDS kernel needs none)."""
    from gct_plus_amd import ops
    hdr = open(os.path.join(ROOT, "include", "gctplus_hip.h")).read()
    limit = int(re.search(r"#define GCT_ATTN_DIRECT_MAX_KEYS (\d+)", hdr).group(1))
    assert limit == ops.ATTN_DIRECT_MAX_KEYS
    lib = _lib.load()
    B, H, Lq = 3, 8, 100
    rows, tiles = B * H * 112, B * H * 7
    assert lib.gct_attn_bwd_ws_bytes(B, H, Lq, limit) == rows * (16 + 4 * limit // 32) + (tiles * 4 + 15) // 16 * 16
    assert lib.gct_attn_bwd_ws_bytes(B, H, Lq, 1) == lib.gct_attn_bwd_ws_bytes(B, H, Lq, limit)
    assert lib.gct_attn_bwd_ws_bytes(B, H, Lq, limit + 1) == 0
    assert lib.gct_attn_bwd_ws_bytes(0, H, Lq, limit) == 0


def test_ops_refuse_cpu_tensors():
    from gct_plus_amd import ops
    with pytest.raises(_lib.GctError):
        ops.norm_fwd(torch.zeros(4, 8), torch.ones(8), torch.zeros(8))


def test_missing_library_is_a_hard_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.GctError):
        _lib.load()


def test_train_flags_match_reference_surface():
    from gct_plus_amd.Configuration.config import train_opts
    p = argparse.ArgumentParser()
    train_opts(p)
    a = p.parse_args("-seed 1 -model_type pscavaetf -lr_WarmUpSteps 15000 -use_cond2lat -use_scaffold "
                     "-start_epoch 1 -num_epoch 50 -batch_size 64 -property_list logP tPSA QED "
                     "-model_folder ./Experiment/x".split())     # Bashscript/train/train_pscavaetf.sh
    assert (a.N, a.H, a.d_ff, a.d_model, a.latent_dim, a.dropout) == (6, 8, 2048, 512, 128, 0.1)
    assert (a.lr, a.lr_beta1, a.lr_beta2, a.lr_eps, a.lr_WarmUpSteps) == (1e-4, 0.9, 0.98, 1e-9, 15000)
    assert (a.KLA_ini_beta, a.KLA_inc_beta, a.KLA_max_beta, a.KLA_beg_epoch) == (0.02, 0.02, 1.0, 1)
    assert a.property_list == ["logP", "tPSA", "QED"] and a.use_cond2lat and not a.use_cond2dec


def test_schedules_match_oracle():
    from gct_plus_amd.Train.trainer1 import KLAnnealer, warmup_lr
    for s in (1, 2, 100, 8000, 20000):
        assert warmup_lr(s, 512, 8000) == O.warmup_lr(s, 512, 8000)
    assert KLAnnealer(1, 0.02, 0.02, 1) == O.kl_beta(1) == pytest.approx(0.04)


def test_masks_match_oracle_and_known_answers():
    from gct_plus_amd.Model import get_src_mask, get_trg_mask, nopeak_mask
    assert nopeak_mask(3, False, 1, 0).tolist() == [[[1, 0, 0], [1, 1, 0], [1, 1, 1]]]
    assert nopeak_mask(2, True, 1, 2).tolist() == [[[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 1]]]
    assert nopeak_mask(3, False, 1, 0).dtype == torch.int64
    ds = synthetic.make_dataset(5, 20, "pscavaetf", seed=3)
    trg_in = ds["trg"][:, :-1]
    assert torch.equal(get_src_mask(ds["src"], 1, ds["econds"]), O.get_src_mask(ds["src"], 1, ds["econds"]))
    assert torch.equal(get_trg_mask(trg_in, 1, False, ds["dconds"]), O.get_trg_mask(trg_in, 1, False, ds["dconds"]))
    assert torch.equal(get_trg_mask(trg_in, 1, True, ds["dconds"]), O.get_trg_mask(trg_in, 1, True, ds["dconds"]))


@pytest.mark.parametrize("mtype", ["vaetf", "pvaetf", "scavaetf", "pscavaetf"])
def test_product_modules_init_and_layout_parity(mtype):
    """Same seed => bit-identical initial weights, same state_dict keys and parameter order as
    the oracle (which is pinned to the reference by tests/golden)."""
    from gct_plus_amd.Model import model_dict
    vs, vt = synthetic.vocab_sizes(mtype)
    nc = synthetic.n_conds(mtype)
    kw = dict(N=2, d_model=64, dff=128, h=4, latent_dim=16)
    torch.manual_seed(1)
    m = model_dict[mtype](vs, vt, dropout=0.0, nconds=nc, use_cond2lat=True, **kw)
    st = O.init_state(O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=nc, use_cond2lat=True, **kw), seed=1)
    sd = m.state_dict()
    assert list(sd) == list(st)
    assert all(torch.equal(sd[k], st[k]) for k in st)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=nc, use_cond2lat=True, **kw)
    assert [n for n, _ in m.named_parameters()] == O.param_names(cfg)


def test_full_size_parameter_counts():
    """SURVEY 8(a) a20 [probe]: 44 514 334 / 44 395 294 / 44 384 543 / 44 396 831 parameters."""
    from gct_plus_amd.Model import model_dict
    exp = {"vaetf": 44514334, "pvaetf": 44395294, "scavaetf": 44384543, "pscavaetf": 44396831}
    for mtype, n in exp.items():
        vs, vt = synthetic.vocab_sizes(mtype)
        m = model_dict[mtype](vs, vt, N=6, d_model=512, dff=2048, h=8, latent_dim=128,
                              nconds=synthetic.n_conds(mtype), use_cond2lat=True)
        assert sum(p.numel() for p in m.parameters()) == n, mtype
        assert len(m.state_dict()) == {"vaetf": 272, "pvaetf": 272, "scavaetf": 268, "pscavaetf": 272}[mtype]


def test_flat_buffers_alias_parameters():
    from gct_plus_amd.Model import model_dict
    torch.manual_seed(0)
    m = model_dict["pvaetf"](28, 30, N=1, d_model=64, dff=128, h=4, latent_dim=16, nconds=3, use_cond2lat=True)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.flatten_parameters()
    flat = m.flat_params()
    for (k, v) in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    p = next(m.parameters())
    flat[:p.numel()] += 1.0
    assert torch.equal(p.detach().flatten(), before[next(iter(before))].flatten() + 1.0)
    for q in m.parameters():
        assert q._gct_gview.shape == q.shape and q._gct_gview.data_ptr() % 16 == 0
    m.sync_grads_to_flat()
    assert all(q.grad is None or q.grad.data_ptr() == q._gct_gview.data_ptr() for q in m.parameters())


def test_shard_indices_match_distributed_sampler():
    from torch.utils.data.distributed import DistributedSampler
    data = list(range(1003))
    for world in (1, 2, 8):
        for rank in range(world):
            for shuffle in (False, True):
                s = DistributedSampler(data, num_replicas=world, rank=rank, shuffle=shuffle, seed=5, drop_last=False)
                s.set_epoch(3)
                assert list(s) == synthetic.shard_indices(len(data), world, rank, epoch=3, seed=5, shuffle=shuffle)


def test_synthetic_layout():
    ds = synthetic.make_dataset(64, 80, "pscavaetf", seed=0)
    assert ds["src"].shape == (64, 80) and ds["trg"].shape == (64, 82) and ds["econds"].shape == (64, 3)
    assert int(ds["src"].max()) < 29 and int(ds["trg"].max()) < 31
    assert (ds["trg"][:, 0] == synthetic.SOS_ID).all() and (ds["src"][0] != synthetic.PAD_ID).all()
    lens = (ds["src"] != 1).sum(1)
    eos = ds["trg"].gather(1, (lens + 1).unsqueeze(1)).squeeze(1)
    assert (eos == synthetic.EOS_ID).all()


def _plan(caller, **kw):
    """engine.plan_rows with the trainer's case as the default: all switches on, loss rows and a target mask, the
    reference's [B, 1, Le] key-padding mask, 6 + 6 layers."""
    from gct_plus_amd import engine
    B, T, Le = kw.pop("B", 4), kw.pop("T", 60), kw.pop("Le", 70)
    args = dict(loss_rows=True, trg_mask=True, n_enc=6, n_dec=6, compact_fwd=True, compact_kv=True,
                compact_enc_kv=True)
    args.update(kw)
    shape = args.pop("mask_shape", (B, 1, Le))
    want = engine.plan_rows(caller, B, T, Le, shape, **args)
    return (want.enc_keys, want.dec_keys, want.live)


def test_row_planner_decision_table():
    """engine.plan_rows: which of the three row maps (encoder keys, decoder memory keys, loss rows) each caller builds.
    The callers keep the rules they had when each decided on its own: the model forward builds nothing with get_attn
    and needs a [B, 1, Le] mask; a decoder on its own (and prefill) still compacts the memory keys with get_attn and
    needs only B * Le mask elements; nothing under stream capture; the encoder on its own builds nothing."""
    from gct_plus_amd import engine, ops
    M, D, P, E = engine.MODEL, engine.DECODER, engine.PREFILL, engine.ENCODER
    K = ops.ATTN_DIRECT_MAX_KEYS
    assert K == 96
    # each caller, the trainer's case
    assert _plan(M) == (True, True, True)
    assert _plan(D) == (False, True, True)
    assert _plan(P, loss_rows=False) == (False, True, False)
    assert _plan(E) == (False, False, False)
    # get_attn: the model forward builds nothing, a decoder alone still maps its memory keys
    assert _plan(M, get_attn=True) == (False, False, False)
    assert _plan(D, get_attn=True) == (False, True, False)
    # cond2dec: no live rows (and T counts the condition rows); without conditions the flag is inert
    assert _plan(M, cond2dec=True, nconds=3) == (True, True, False)
    assert _plan(D, cond2dec=True, nconds=3) == (False, True, False)
    assert _plan(M, cond2dec=True, nconds=0) == (True, True, True)
    w = engine.plan_rows(M, 4, 60, 70, (4, 1, 70), cond2dec=True, cond2lat=True, nconds=3)
    assert (w.nc_lat, w.live_rows, w.dec_rows) == (0, 4 * 63, 4 * 70)
    # cond2lat: the decoder's memory has nconds visible rows in front; they count against the key limit
    w = engine.plan_rows(M, 4, 60, 70, (4, 1, 70), cond2lat=True, nconds=3, compact_kv=True)
    assert (w.nc_lat, w.enc_rows, w.dec_rows, w.live_rows) == (3, 4 * 70, 4 * 73, 4 * 60)
    for c in (M, D):
        assert _plan(c, Le=K - 3, mask_shape=(4, 1, K - 3), cond2lat=True, nconds=3)[2]
        assert not _plan(c, Le=K - 2, mask_shape=(4, 1, K - 2), cond2lat=True, nconds=3)[2]
        assert _plan(c, Le=K - 2, mask_shape=(4, 1, K - 2), cond2lat=True, nconds=3)[1]    # keys have no limit
    # T and Le + nc_lat at the direct kernels' key limit, 96, and one above
    for c in (M, D):
        assert _plan(c, T=K)[2] and not _plan(c, T=K + 1)[2]
        assert _plan(c, Le=K, mask_shape=(4, 1, K))[2] and not _plan(c, Le=K + 1, mask_shape=(4, 1, K + 1))[2]
        assert _plan(c, T=K - 3, cond2dec=True, nconds=3)[2] is False                 # (cond2dec: never)
    assert _plan(M, T=K + 1) == (True, True, False) and _plan(D, Le=K + 1, mask_shape=(4, 1, K + 1)) == (False, True, False)
    # switches off, one at a time
    assert _plan(M, compact_fwd=False) == (True, True, False)
    assert _plan(M, compact_kv=False) == (True, False, True)
    assert _plan(M, compact_enc_kv=False) == (False, True, True)
    assert _plan(D, compact_kv=False) == (False, False, True)
    assert _plan(D, compact_enc_kv=False) == (False, True, True)
    # stream capture: nothing, for every caller
    for c in (M, D, P, E):
        assert _plan(c, capturing=True) == (False, False, False)
    # no target mask / no loss rows: no live rows
    for c in (M, D):
        assert not _plan(c, trg_mask=False)[2] and not _plan(c, loss_rows=False)[2]
    # the key-padding mask: the model forward wants [B, 1, Le]; a decoder alone any shape of B * Le elements
    assert _plan(M, mask_shape=(4, 70)) == (False, False, False)
    assert _plan(M, mask_shape=(4, 60, 70)) == (False, False, False)
    assert _plan(M, mask_shape=None) == (False, False, False)
    assert _plan(D, mask_shape=(4, 70)) == (False, True, True)
    assert _plan(D, mask_shape=(4, 1, 70)) == (False, True, True)
    assert _plan(D, mask_shape=(4, 60, 70)) == (False, False, True)
    assert _plan(D, mask_shape=None) == (False, False, True)
    assert _plan(P, mask_shape=(4, 60, 70), loss_rows=False) == (False, False, False)
    # zero layers
    assert _plan(M, n_enc=0) == (False, True, True)
    assert _plan(M, n_dec=0) == (True, False, False)
    assert _plan(D, n_dec=0) == (False, False, False)
    with pytest.raises(ValueError):
        _plan("trainer")


def test_row_map_usable_tests():
    """RowPlan.usable_keys / usable_live, pure functions of a map's host info record: exact (every prefix, no
    violation, no empty sample for keys) and worth it (0 < compact rows <= COMPACT_MAX_FRACTION of all rows)."""
    from gct_plus_amd import engine
    assert engine.COMPACT_MAX_FRACTION == 0.85
    rows = 1000
    h = dict(n_live=500, violations=0, nonprefix=0, tiles=20, padded=512, quads=128, empty=0)
    keys, live = engine.RowPlan.usable_keys, engine.RowPlan.usable_live
    assert keys(h, rows) and live(h, rows)
    assert keys(dict(h, padded=850), rows) and live(dict(h, padded=850), rows)              # at the boundary
    assert not keys(dict(h, padded=852), rows) and not live(dict(h, padded=852), rows)      # above it
    assert not keys(dict(h, padded=0), rows) and not live(dict(h, padded=0), rows)          # nothing left
    assert not keys(dict(h, nonprefix=1), rows) and not live(dict(h, nonprefix=1), rows)    # a non-prefix mask
    assert not live(dict(h, violations=1), rows) and keys(dict(h, violations=1), rows)      # (keys: no such check)
    assert not keys(dict(h, empty=1), rows) and live(dict(h, empty=1), rows)                # (live: no such check)


class _FakeMap:
    """A row map whose info record is already on the host (no device work in RowPlan / PendingReadBack)."""

    def __init__(self, padded):
        self._host = dict(n_live=8, violations=0, nonprefix=0, tiles=1, padded=padded, quads=2, empty=0)

    def host(self):
        return self._host


def test_row_plan_finish(monkeypatch):
    """RowPlan.finish(): keeps the usable maps, can be called more than once, and a plan finished under stream capture
    keeps its key maps but not its live map (the decoder then runs on every row)."""
    from gct_plus_amd import engine
    ek, dk, lr, bad = _FakeMap(8), _FakeMap(8), _FakeMap(8), _FakeMap(0)
    plan = engine.RowPlan(ek, dk, lr, (16, 16, 16))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert plan.finish() is plan
    assert (plan.enc_keys, plan.dec_keys, plan.live) == (ek, dk, lr) and lr.fwd is True
    assert plan.finish() is plan and (plan.enc_keys, plan.dec_keys, plan.live) == (ek, dk, lr)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert (plan.finish().enc_keys, plan.dec_keys, plan.live) == (ek, dk, None)
    plan = engine.RowPlan(bad, dk, bad, (16, 16, 16)).finish()
    assert (plan.enc_keys, plan.dec_keys, plan.live) == (None, dk, None)
    empty = engine.RowPlan().finish()
    assert (empty.enc_keys, empty.dec_keys, empty.live) == (None, None, None)
