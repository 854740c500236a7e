"""Int8 weight-only quantization through the SIMT emulator (CPU): quantizer, format, dequant / GEMV kernels, the int8 decode engine
against the dequantizing tile path, prefill equivalence, the generate surface (tests/quant_cases.py)."""
import pytest

from tests import quant_cases as Q

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def emu():
    from tests.emu import emu_lib

    emu_lib.install()
    yield
    emu_lib.uninstall()


def test_quantizer():
    Q.case_quantizer()


def test_state_dict_layout_and_round_trip():
    Q.case_state_dict_layout()


def test_quantized_model_is_inference_only():
    Q.case_quantized_is_inference_only()


def test_aria_width_bytes():
    Q.case_aria_width_bytes()


def test_dequant():
    Q.case_dequant(DEV)


def test_gemv():
    Q.case_gemv(DEV, Ks=(2560, 136, 1000), Ns=(37, 300))


def test_gemv_head_rows():  # N >= 32768: the 8-rows-per-wave form of the output head
    Q.case_gemv(DEV, Ks=(136,), Ns=(32800,))


@pytest.mark.parametrize("head_dim", [64, 128])
def test_engine_vs_tile_path(head_dim):
    Q.case_engine_vs_tile(DEV, head_dim)


def test_prefill_equivalence():
    Q.case_prefill_equivalence(DEV)


def test_generate():
    Q.case_generate(DEV)


def test_generator_from_int8_checkpoint(tmp_path):
    Q.case_generator_from_int8_checkpoint(DEV, tmp_path)


def test_bf16_load_unchanged():
    Q.case_bf16_load_unchanged(DEV)


def test_head_wide_falls_back_to_dequant():
    Q.case_head_wide(DEV)


def test_engine_aria_width_vs_oracle():
    Q.case_engine_aria_width(DEV, n_tokens=2)
