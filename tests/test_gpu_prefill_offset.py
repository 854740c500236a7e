"""Prefill at a cache offset on the MI355X (tests/prefill_offset_cases.py): the offset attention launch against the fp32 oracle (also at
the real head count), the gptfast continuation path at toy and Aria widths, generate's prefill_chunk / cached_prefix, Generator's
reuse_prefix."""
import pytest

from tests import prefill_offset_cases as P
from tests.test_emu_prefill_offset import SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_oracle(shape, hd):
    B, H, Sq, q_off, Skv = shape
    P.case_kernel(DEV, B, H, Sq, q_off, Skv, hd)


def test_kernel_real_head_count():
    P.case_kernel(DEV, 1, 20, 512, 2061, 2573, 128)


@pytest.mark.parametrize("hd", [128, 64])
def test_kernel_grouped_block_order(hd, monkeypatch):
    monkeypatch.setenv("ARIA_ATTN_CAUSAL_GROUPED", "1")
    P.case_kernel(DEV, 2, 2, 300, 77, 448, hd)


@pytest.mark.parametrize("hd", [128, 64])
def test_kernel_kv_len(hd):
    P.case_kernel(DEV, 2, 2, 300, 77, 448, hd, kv_len=[377, 350])


@pytest.mark.parametrize("hd", [128, 64])
def test_zero_offset_is_plain_causal(hd):
    P.case_zero_offset_is_plain_causal(DEV, hd)


def test_validation():
    P.case_validation(DEV)


@pytest.mark.parametrize("head_dim", [64, 128])
def test_model_continuation(head_dim):
    P.case_model_continuation(DEV, head_dim)


def test_model_continuation_int8():
    P.case_model_continuation(DEV, 64, int8=True)


def test_model_continuation_batch2():
    P.case_model_batch2(DEV)


def test_model_errors():
    P.case_model_errors(DEV)


def test_aria_width_chunks():
    P.case_aria_width_chunks(DEV)


def test_generate_chunked():
    P.case_generate_chunked(DEV)


def test_generate_cached_prefix():
    P.case_generate_cached_prefix(DEV)


def test_generator_reuse_prefix():
    P.case_generator_reuse(DEV)
