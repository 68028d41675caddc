"""CPU-only tests of the host side: C-ABI symbol table, flag surface, schedules, data sharding,
mask builders, init-order parity of the product modules, flat-buffer bookkeeping."""
import argparse
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from gct_plus_amd import _lib, synthetic
from oracle import gct_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exported_gct_symbols(path):
    """The unmangled gct_* names a shared object defines (the C++-mangled helpers shared between translation units
    start with _Z and do not count)."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("gct_")}


def test_library_exports_every_declared_symbol():
    """include/gctplus_hip.h <-> _lib.SIGNATURES (parsed from it) <-> the built .so (no compute call).  The name regex
    below is independent of _lib's parser: a prototype the parser drops shows up here."""
    hdr = open(os.path.join(ROOT, "include", "gctplus_hip.h")).read()
    declared = set(re.findall(r"\b(gct_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    header_version = int(re.search(r"^#define GCT_ABI_VERSION (\d+)$", hdr, flags=re.M).group(1))
    assert header_version == lib.gct_version() == _lib.ABI_VERSION
    assert lib.gct_wgrad_ws_bytes(40960, 512, 512) > 0
    # the diagnostics library has its own header and is NOT part of the operator ABI
    dh = open(os.path.join(ROOT, "include", "gctplus_diag.h")).read()
    ddecl = set(re.findall(r"\b(gct_[a-z0-9_]+)\s*\(", dh))
    assert ddecl == set(_lib.DIAG_SIGNATURES) and not (ddecl & declared), (ddecl, declared & ddecl)
    dl = _lib.load_diag()
    for name, (res, args) in _lib.DIAG_SIGNATURES.items():
        fn = getattr(dl, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # both directions: the libraries define no gct_* symbol that their header does not declare
    if shutil.which("nm"):
        assert _exported_gct_symbols(_lib.LIB_PATH) == declared
        assert _exported_gct_symbols(_lib.DIAG_PATH) == ddecl


def test_header_parser_on_a_literal_header():
    """_lib.parse_prototypes alone: one prototype per supported type, pointers by the two pointer rules, a prototype over
    several lines, (void), comments that look like calls, a struct typedef; an unknown value type or text that is no
    prototype raises and names it -- nothing is bound by default."""
    C = ctypes
    text = """
    /* gct_in_a_comment(int a); is not a prototype */
    #ifndef X_H
    #define X_H
    #define GCT_ABI_VERSION 7   /* gct_define(1) */
    #ifdef __cplusplus
    extern "C" {
    #endif
    // gct_line_comment(float x);
    typedef struct GctThing { int32_t k; float p; } GctThing;
    int gct_version(void);
    const char* gct_last_error(void);
    int64_t gct_bytes(int64_t M, int K, int32_t n, float p, uint64_t seed, uint32_t site);
    int gct_many(const float* x, int64_t ldx,   /* gct_inside(2) */
                 float* y, const uint16_t* planes, const int64_t* tok,
                 const int32_t* map, uint8_t* live, void* stream,
                 const GctThing* thing);
    int gct_strings(const char* s, char* buf, const char* const* names, const int64_t* const* rows);
    #ifdef __cplusplus
    }
    #endif
    #endif
    """
    P, I, I64 = C.c_void_p, C.c_int, C.c_int64
    assert _lib.parse_prototypes(text) == {
        "gct_version": (I, []),
        "gct_last_error": (C.c_char_p, []),
        "gct_bytes": (I64, [I64, I, C.c_int32, C.c_float, C.c_uint64, C.c_uint32]),
        "gct_many": (I, [P, I64, P, P, P, P, P, P, P]),
        "gct_strings": (I, [C.c_char_p, C.c_char_p, P, P]),
    }
    for bad, named in (("int gct_a(double x);", "gct_a"), ("double gct_b(int x);", "gct_b"),
                       ("int gct_c(unsigned int n);", "gct_c"), ("int gct_d(size_t n);", "gct_d"),
                       ("int gct_e(int (*cb)(int));", "cb"), ("int gct_f(int a)", "gct_f")):
        with pytest.raises(_lib.GctError, match=named):
            _lib.parse_prototypes("int gct_ok(int a);\n" + bad)


def test_missing_header_is_a_hard_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "INCLUDE_DIR", str(tmp_path))
    with pytest.raises(_lib.GctError):
        _lib._parse_header("gctplus_hip.h")
    (tmp_path / "gctplus_hip.h").write_text("/* nothing declared */\n")
    with pytest.raises(_lib.GctError):
        _lib._parse_header("gctplus_hip.h")
    with pytest.raises(_lib.GctError):
        _lib._abi_version()


def test_saved_state_is_read_by_name():
    """The records a forward saves for its backward (engine.MhaSaved ... DecoderSaved) have one owner of their layout:
    nothing in the package indexes them by position."""
    pat = re.compile(r"saved\[\d|\bsv\[\d|\bsv1\[|\bsv2\[|\bsvf\[|\blsv\b[^\n]*\]\[-1\]")
    hits = []
    pkg = os.path.join(ROOT, "gct_plus_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                for no, line in enumerate(open(os.path.join(d, f), encoding="utf-8"), 1):
                    if pat.search(line):
                        hits.append(f"{os.path.relpath(os.path.join(d, f), ROOT)}:{no}: {line.strip()}")
    assert not hits, hits
    assert not pat.search("prefix = (sv[:, :-1] >= sv[:, 1:]).all(1)")          # decode.py's mask tensor
    for line in ("x = saved[4]", "q = sv[3][2]", "s = sv[11]", "a = sv1[2]", "b = sv2[0]", "c = svf[4]",
                 "below=lsv[i - 1][-1] if i > 0 else None"):
        assert pat.search(line), line


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
