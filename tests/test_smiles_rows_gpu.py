"""The launch prelude of the SMILES kernels on the device (smiles.launch_rows): each of the six *_rows methods gives the
same tensors for starts on the host, the same starts as an int32 tensor on the device and an int32, column-strided ys --
and they equal the module's *_reference on the rows of the host test's table whose start lies inside [0, W]."""
import pytest
import torch

from gct_plus_amd import ops as _ops
from tests.test_smiles_rows_host import CHEM, DESC, FPS, IN_RANGE, KEYS, RZ, SCA, STARTS, W, YS

pytestmark = pytest.mark.gpu

ROWS, START = YS[IN_RANGE], [STARTS[r] for r in IN_RANGE]
KEY, SEED = torch.arange(len(START)) * 7 + 1, 5
CALLS = {
    "keys": (KEYS.key_rows, KEYS.key_reference, {}),
    "fingerprints": (FPS.fp_rows, FPS.fp_reference, {}),
    "descriptors": (DESC.desc_rows, DESC.desc_reference, {}),
    "scaffolds": (SCA.scaffold_rows, SCA.scaffold_reference, {}),
    "randomiser": (lambda ys, st, **kw: RZ.randomize_rows(ys, st, KEY, SEED, **kw),
                   lambda ys, st, **kw: RZ.randomize_reference(ys, st, KEY, SEED, **kw), {"return_perm": True}),
}


@pytest.fixture(scope="module")
def ops():
    _ops._L()
    return _ops


def strided_int32(ys):
    """ys as an int32 view with a column stride of 2 on the device."""
    wider = torch.full((ys.shape[0], 2 * ys.shape[1]), -1, dtype=torch.int32)
    wider[:, ::2] = ys.to(torch.int32)
    view = wider.cuda()[:, ::2]
    assert view.stride(1) == 2 and view.dtype == torch.int32
    return view


def same(got, want, what):
    assert type(got) is type(want), what
    for name, a, b in zip(want._fields, got, want):
        assert a.is_cuda and a.dtype == b.dtype and torch.equal(a.cpu(), b), (what, name, a.cpu().tolist(), b.tolist())


@pytest.mark.parametrize("which", list(CALLS))
def test_three_ways_to_pass_rows_give_the_reference(ops, which):
    rows, reference, kw = CALLS[which]
    assert ROWS.shape == (9, W) and W in START and 0 in START
    want = reference(ROWS, START, **kw)
    dev = ROWS.cuda()
    same(rows(dev, torch.tensor(START, dtype=torch.int64), **kw), want, "int64 starts on the host")
    same(rows(dev, torch.tensor(START, dtype=torch.int32, device="cuda"), **kw), want, "int32 starts on the device")
    same(rows(strided_int32(ROWS), START, **kw), want, "int32 rows with a column stride of 2")


def test_check_rows_stands_apart(ops):
    """No device-start path: prefix_lens are checked on the host whatever holds them."""
    want = CHEM.check_reference(ROWS, START)
    same(CHEM.check_rows(ROWS.cuda(), torch.tensor(START, dtype=torch.int64)), want, "int64 prefix_lens on the host")
    same(CHEM.check_rows(strided_int32(ROWS), START), want, "int32 rows with a column stride of 2")
    same(CHEM.check_rows(ROWS.cuda(), torch.tensor(START, dtype=torch.int32, device="cuda")), want, "device prefix_lens")
    with pytest.raises(ValueError, match="prefix_lens must lie in"):
        CHEM.check_rows(ROWS.cuda(), torch.tensor([W + 1] * len(START), dtype=torch.int32, device="cuda"))
