"""The full sampler on the MI355X (tests/sample_cases.py): aria_sample / aria_token_bitmap against the float64 oracle, and the top_p / min_p /
repetition_penalty / logprobs options of the gptfast surface."""
import pytest

from tests import sample_cases as S
from tests.test_emu_sample import VOCABS

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("largest log-prob error seen:", S.OBSERVED["logprob_err"])


@pytest.mark.parametrize("sigma", [1.0, 4.0])
@pytest.mark.parametrize("V", VOCABS)
def test_vocabulary_sizes(V, sigma):
    S.case_vocab(DEV, V, sigma)


def test_peaked():
    S.case_peaked(DEV)


def test_all_logits_equal():
    S.case_all_equal(DEV)


def test_two_distinct_values():
    S.case_two_values(DEV)


def test_filter_interplay():
    S.case_interplay(DEV)


def test_penalty():
    S.case_penalty(DEV)


def test_update_seen():
    S.case_update_seen(DEV)


@pytest.mark.parametrize("V", VOCABS)
def test_neutral_options_are_sample_topk(V):
    S.case_neutral(DEV, V)


def test_determinism():
    S.case_determinism(DEV)


def test_validation():
    S.case_validation(DEV)


@pytest.mark.parametrize("opts", S.OPTION_SETS, ids=["top_p", "min_p"])
def test_generate_vs_oracle(opts):
    S.case_generate_vs_oracle(DEV, opts)


def test_generate_options():
    S.case_generate_options(DEV)


def test_generator_turns():
    S.case_generator_turns(DEV)


def test_hf_generate(golden):
    S.case_hf_generate(DEV, golden)
