"""What the encoder sees, per sampler type: encode_smiles, score_smiles(zs=None) and the endpoint encoding of
interpolate_smiles / reconstruct_smiles must hand the model the same (src, src_mask, econds).  No GPU: the tiny CPU
samplers of test_mixed_scaffold_host, with model.encode replaced by a recorder."""
import numpy as np
import pytest
import torch

from gct_plus_amd import data
from gct_plus_amd.Inference.sampling_tool import CvaetfSampling, PscavaetfSampling, ScaVaeSampling, VaetfSampling
from tests.test_data_pipeline import SMILES
from tests.test_mixed_scaffold_host import TINY, make_sampler

MOLS = SMILES[:4]
SCAFFOLDS = ["c1ccccc1", "C1CC1", "c1ccc2ccccc2c1", "CC"]                      # 8, 5, 14 and 2 tokens
PROPS = np.arange(12, dtype=np.float32).reshape(4, 3) / 7


class Recorder:
    """Stands in for model.encode: keeps every (src, src_mask, econds) it is handed, returns zeros (z, mu, log_var)."""

    def __init__(self):
        self.calls = []

    def __call__(self, src, src_mask, econds=None):
        self.calls.append((src.clone(), src_mask.clone(), None if econds is None else econds.clone()))
        z = torch.zeros(src.shape[0], src_mask.shape[-1], TINY["latent_dim"])
        return z, z.clone(), z.clone()


@pytest.mark.parametrize("cls, mtype", [(VaetfSampling, "vaetf"), (CvaetfSampling, "pvaetf"),
                                        (ScaVaeSampling, "scavaetf"), (PscavaetfSampling, "pscavaetf")])
def test_every_entry_point_hands_the_encoder_the_same_inputs(cls, mtype):
    sp = make_sampler(cls, mtype)
    rec = sp.model.encode = Recorder()
    sp.score = lambda *a, **k: None                        # the scoring forward itself needs the device
    sca = SCAFFOLDS if sp.uses_scaffold else None
    props = PROPS if sp.uses_props else None
    args = [MOLS] + ([sca] if sp.uses_scaffold else []) + ([props] if sp.uses_props else [])
    kw = {"transform": False} if sp.uses_props else {}
    sp.encode_smiles(*args, **kw)
    sp.score_smiles(*args, zs=None, **kw)
    _, _, mask = sp._encode_endpoints(MOLS, sca, None if props is None else props.astype(np.float64), False)
    assert len(rec.calls) == 3
    src, src_mask, econds = rec.calls[0]
    # (a) the three entry points: bit-identical inputs
    for other in rec.calls[1:]:
        assert torch.equal(other[0], src) and other[0].dtype == src.dtype
        assert torch.equal(other[1], src_mask) and other[1].dtype == src_mask.dtype
        assert (econds is None) == (other[2] is None)
        if econds is not None:
            assert torch.equal(other[2], econds) and other[2].dtype == econds.dtype
    assert torch.equal(mask, src_mask)
    # (b) src: the tokens of scaffold<sep>smiles (scaffold types) or of smiles, right-padded
    strings = [b + "<sep>" + a for a, b in zip(MOLS, SCAFFOLDS)] if sp.uses_scaffold else MOLS
    rows = [[sp.SRC.stoi[t] for t in data.tokenize(s, sp.add_sep)] for s in strings]
    L = max(len(r) for r in rows)
    assert src.dtype == torch.int64
    assert src.tolist() == [r + [sp.pad_id] * (L - len(r)) for r in rows]
    # (c) src_mask [n, 1, n_c + L]: the n_c condition flags set (property types), then one flag per token
    nc = 3 if sp.uses_props else 0
    assert src_mask.dtype == torch.bool and tuple(src_mask.shape) == (4, 1, nc + L)
    assert bool(src_mask[:, :, :nc].all())
    assert src_mask[:, 0, nc:].tolist() == [[True] * len(r) + [False] * (L - len(r)) for r in rows]
    if sp.uses_props:
        assert econds.dtype == torch.float32 and torch.equal(econds, torch.as_tensor(PROPS))
    else:
        assert econds is None
