"""ISA guards of the int8 weight-only decode kernels (csrc/decode.hip, *_w8): no scratch, the weight rows are 8-byte non-temporal global
loads, and no `s_waitcnt vmcnt(0)` between the first weight load and the activation vector fetch (the rows' HBM latency must hide the
vector's, as in the bf16 engine).  CPU only: hipcc cross-compiles gfx950."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

KERNELS = ("gemv_w8_kernelILi2ELi5", "gemv_w8_kernelILi4ELi5", "gemv_w8_kernelILi8ELi5", "router_shared_up_w8_kernelILi2ELi5",
           "expert_up_w8_kernelILi4ELi5", "expert_down_combine_w8_kernelILi4ELi7")
_ISA = []


def isa():
    if not _ISA:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Iinclude", "-Iaria_amd/csrc", "-S", "--cuda-device-only",
                            os.path.join("aria_amd", "csrc", "decode.hip"), "-o", "-"], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _ISA.append(r.stdout.split("\n"))
    return _ISA[0]


def body(frag):
    lines = isa()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(frag) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end], "\n".join(lines[end:end + 400])


@pytest.mark.parametrize("frag", KERNELS)
def test_no_scratch(frag):
    b, meta = body(frag)
    assert not any("scratch_" in l for l in b), frag
    m = re.search(r"\.private_segment_fixed_size:\s*(\d+)", meta) or re.search(r"ScratchSize:\s*(\d+)", meta)
    assert m is None or int(m.group(1)) == 0, frag


@pytest.mark.parametrize("frag", KERNELS)
def test_weight_loads_are_nt_dwordx2(frag):
    b, _ = body(frag)
    loads = [l for l in b if "global_load_dwordx2" in l]
    assert loads and all(l.rstrip().endswith(" nt") for l in loads), frag


@pytest.mark.parametrize("frag", [k for k in KERNELS if "down_combine" not in k])
def test_no_full_drain_before_vector(frag):
    """between the first weight load and the first 16-byte vector load (load_vector) nothing waits for every load to land"""
    b, _ = body(frag)
    first_w = next(i for i, l in enumerate(b) if "global_load_dwordx2" in l)
    first_v = next(i for i in range(first_w, len(b)) if "global_load_dwordx4" in b[i])
    assert not any(re.search(r"s_waitcnt\s+vmcnt\(0\)", l) for l in b[first_w:first_v]), frag
