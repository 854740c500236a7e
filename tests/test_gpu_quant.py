"""Int8 weight-only quantization on the MI355X (tests/quant_cases.py): the kernels at Aria's shapes, the int8 decode engine against the
dequantizing tile path, prefill equivalence, the generate surface."""
import pytest

from tests import quant_cases as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_dequant():
    Q.case_dequant(DEV)


def test_dequant_aria_expert_tensor():
    Q.case_dequant_expert_tensor(DEV)


def test_gemv():
    Q.case_gemv(DEV)


def test_gemv_head_rows():  # the output head's shape: 100 352 rows, 8 per wave
    Q.case_gemv(DEV, Ks=(2560,), Ns=(100352,))


@pytest.mark.parametrize("head_dim", [64, 128])
def test_engine_vs_tile_path(head_dim):
    Q.case_engine_vs_tile(DEV, head_dim)


@pytest.mark.parametrize("head_dim", [64, 128])
def test_prefill_equivalence(head_dim):
    Q.case_prefill_equivalence(DEV, head_dim)


def test_generate():
    Q.case_generate(DEV)


def test_generator_from_int8_checkpoint(tmp_path):
    Q.case_generator_from_int8_checkpoint(DEV, tmp_path)


def test_bf16_load_unchanged():
    Q.case_bf16_load_unchanged(DEV)


def test_head_wide_falls_back_to_dequant():
    Q.case_head_wide(DEV)


def test_engine_aria_width_vs_oracle():
    Q.case_engine_aria_width(DEV, n_tokens=6)


def test_engine_full_depth_28_layers():
    """config #2's path at 28 layers on an int8 model: prefill 280, 16 greedy int8-engine steps against the routing-forced fp32 oracle"""
    rep = Q.case_engine_full_depth(DEV)
    assert len(rep["tokens"]) == 16
