"""The wide dense pass 1 (csrc/traj_kernels.hip: k_traj_pass1_dense16, sixteen points per lane) is launched with as many blocks
as the host's residency rule (dense_per_cu) says are resident at once; the rule needs an upper bound on the kernel's SGPR count
that the runtime cannot tell: TO_WIDE_SGPRS, declared next to the kernel.  The library's translation unit is compiled for gfx950
as tests/test_dense_resources_cpu.py does it (device code only, no GPU needed): exactly one wide kernel, no scratch, its
registers within the declared bounds (three waves per SIMD: at most 168 VGPRs), and the narrow kernels still there."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "trajectory_optimization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
WIDE, NARROW = "k_traj_pass1_dense16", ("k_traj_pass1_denseILb0E", "k_traj_pass1_denseILb1E")
WAVES_PER_SIMD = 3   # __launch_bounds__(256, 3)
MAX_VGPRS = 512 // WAVES_PER_SIMD // 8 * 8


def by_sgpr(s):
    """Blocks per CU the scalar register file admits at s SGPRs (the host's rule)."""
    return 800 // ((s + 15) // 16 * 16 + 16)


@pytest.fixture(scope="module")
def declared():
    with open(os.path.join(CSRC, "traj_kernels.hip")) as f:
        found = re.findall(r"^#define[ \t]+TO_WIDE_SGPRS[ \t]+(\d+)\b", f.read(), flags=re.M)
    assert len(found) == 1, found
    return int(found[0])


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """kernel name -> {field: int} of the code object's metadata (.sgpr_count, .vgpr_count, .private_segment_fixed_size, ...)."""
    out = str(tmp_path_factory.mktemp("dense_wide_res") / "trajopt.s")
    subprocess.check_call([HIPCC, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "trajopt_hip.hip"), "-o", out], stderr=subprocess.DEVNULL)
    kernels, cur = {}, None
    with open(out) as f:
        for line in f:
            m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", line)
            if not m:
                continue
            if m.group(1) == "name" and m.group(2).startswith("_Z"):
                cur = kernels.setdefault(m.group(2), {})
            elif cur is not None and re.fullmatch(r"\d+", m.group(2)):
                cur.setdefault(m.group(1), int(m.group(2)))
    return {n: m for n, m in kernels.items() if "sgpr_count" in m}


def test_the_declared_bound_admits_the_waves_the_kernel_is_built_for(declared):
    assert by_sgpr(declared) >= WAVES_PER_SIMD, declared


def test_one_wide_kernel_within_its_declared_bounds(metadata, declared):
    names = [n for n in metadata if WIDE in n]
    assert len(names) == 1, names
    m = metadata[names[0]]
    print({f: m[f] for f in ("sgpr_count", "vgpr_count", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0
    assert m["sgpr_count"] <= declared
    assert m["vgpr_count"] <= MAX_VGPRS


def test_the_narrow_kernels_are_still_there(metadata):
    for prefix in NARROW:
        assert len([n for n in metadata if prefix in n]) == 1, prefix
