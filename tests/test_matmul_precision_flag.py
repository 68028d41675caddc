"""CPU: the train1 flag of the opt-in bf16x3 GEMM mode (-matmul_precision {highest,high}, default highest)."""
import argparse

import pytest

from gct_plus_amd.Configuration.config import train_opts

BASE = ["-model_type", "vaetf", "-model_folder", "/nonexistent"]


def parse(extra):
    p = argparse.ArgumentParser()
    train_opts(p)
    return p.parse_args(BASE + extra)


def test_matmul_precision_defaults_to_highest():
    assert parse([]).matmul_precision == "highest"


@pytest.mark.parametrize("value", ["highest", "high"])
def test_matmul_precision_accepts_the_two_tiers(value):
    assert parse(["-matmul_precision", value]).matmul_precision == value


@pytest.mark.parametrize("value", ["medium", "x3", "HIGH", ""])
def test_matmul_precision_rejects_other_values(value):
    with pytest.raises(SystemExit):
        parse(["-matmul_precision", value])


def test_gemm_mode_constants():
    from gct_plus_amd import ops
    assert (ops.GEMM_F32, ops.GEMM_BF16X6, ops.GEMM_BF16X3) == (0, 1, 2)
