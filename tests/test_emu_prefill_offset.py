"""Prefill at a cache offset through the SIMT emulator (CPU): the offset attention launch against the fp32 oracle, the gptfast
continuation path, generate's prefill_chunk / cached_prefix, Generator's reuse_prefix (tests/prefill_offset_cases.py); and the ISA guard of
the new hd-128 kernel (no scratch)."""
import os
import re
import shutil
import subprocess

import pytest

from tests import prefill_offset_cases as P

DEV = "cpu"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (B, H, Sq, q_off, Skv)
SHAPES = [(1, 2, 37, 91, 200),    # neither offset nor length on a tile or wave boundary
          (1, 1, 1, 64, 65),      # one query, offset on a tile boundary
          (1, 2, 5, 700, 705),    # long prefix, most waves of the block hold no query
          (2, 2, 300, 77, 448),   # two query blocks, batch stride larger than the live length
          (1, 2, 64, 192, 256)]   # everything aligned, the diagonal starts exactly at a tile edge


@pytest.fixture(scope="module", autouse=True)
def emu():
    from tests.emu import emu_lib

    emu_lib.install()
    yield
    emu_lib.uninstall()


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_oracle(shape, hd):
    B, H, Sq, q_off, Skv = shape
    P.case_kernel(DEV, B, H, Sq, q_off, Skv, hd)


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


def test_generate_chunked():
    P.case_generate_chunked(DEV)


def test_generate_cached_prefix():
    P.case_generate_cached_prefix(DEV)


def test_generator_reuse_prefix():
    P.case_generator_reuse(DEV)


def test_reusable_prefix():
    P.case_reusable_prefix()


def test_generator_image_bookkeeping():
    P.case_generator_image_bookkeeping()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_offset_kernels_no_scratch():
    """attn_fwd3_off_kernel<128, 8, true> sits at the register budget of two waves per SIMD: the offset must not push it into scratch
    (checked the way tests/test_isa_guards_w8.py::test_no_scratch does)"""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Iinclude", "-Iaria_amd/csrc", "-S", "--cuda-device-only",
                        os.path.join("aria_amd", "csrc", "attn.hip"), "-o", "-"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    for frag in ("20attn_fwd3_off_kernelILi128ELi8ELb1", "20attn_fwd2_off_kernelILi128ELi8", "20attn_fwd2_off_kernelILi64ELi8"):
        start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(frag) + r"\w*:", l))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        meta = "\n".join(lines[end:end + 400])
        assert not any("scratch_" in l for l in lines[start:end]), frag
        m = re.search(r"\.private_segment_fixed_size:\s*(\d+)", meta) or re.search(r"ScratchSize:\s*(\d+)", meta)
        assert m is None or int(m.group(1)) == 0, frag
        v = re.search(r"NumVgprs:\s*(\d+)", meta)
        assert v is None or int(v.group(1)) <= 256, (frag, v.group(1))   # two waves per SIMD
