"""The dense pass 1's grid is sized by the host's residency rule (csrc/traj_kernels.hip: dense_per_cu), which needs an upper bound
on each build's SGPR count that the runtime cannot tell: TO_DENSE_SGPRS and TO_DENSE_OCC_SGPRS, declared next to the kernel.
The library's translation unit is compiled for gfx950 the way tools/kernel_resources.py does it (device code only, no GPU needed)
and both builds are held to what is declared — a count above the bound would let the host launch a block that is not resident
from the start — and to the waves per SIMD they reach today: a change that silently costs the kernel a wave fails here."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "trajectory_optimization_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# build -> (mangled-name prefix, the declared SGPR bound, waves per SIMD = 256-thread blocks per CU the build's registers admit)
BUILDS = {"plain": ("k_traj_pass1_denseILb0E", "TO_DENSE_SGPRS", 6),
          "occlusion": ("k_traj_pass1_denseILb1E", "TO_DENSE_OCC_SGPRS", 5)}


def by_sgpr(s):
    """Blocks per CU the scalar register file admits at s SGPRs (the host's rule)."""
    return 800 // ((s + 15) // 16 * 16 + 16)


@pytest.fixture(scope="session")
def declared():
    with open(os.path.join(CSRC, "traj_kernels.hip")) as f:
        return {k: int(v) for k, v in re.findall(r"^#define[ \t]+(TO_DENSE_\w*SGPRS)[ \t]+(\d+)[ \t]*$", f.read(), flags=re.M)}


@pytest.fixture(scope="session")
def metadata(tmp_path_factory):
    """kernel name -> {field: int} of the code object's metadata (.sgpr_count, .vgpr_count, .private_segment_fixed_size, ...)."""
    out = str(tmp_path_factory.mktemp("dense_res") / "trajopt.s")
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
    return kernels


def test_the_declared_bounds_admit_the_waves_the_builds_reach(declared):
    assert set(declared) == {"TO_DENSE_SGPRS", "TO_DENSE_OCC_SGPRS"}
    for _, sgprs, k in BUILDS.values():
        assert by_sgpr(declared[sgprs]) >= k, (sgprs, declared[sgprs], k)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_compiled_registers_match_the_declared_bounds(metadata, declared, build):
    prefix, sgprs, k = BUILDS[build]
    names = [n for n in metadata if prefix in n and "sgpr_count" in metadata[n]]
    assert len(names) == 1, names
    m = metadata[names[0]]
    print(build, {f: m[f] for f in ("sgpr_count", "vgpr_count", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0
    assert m["sgpr_count"] <= declared[sgprs]
    assert m["vgpr_count"] <= 512 // k // 8 * 8
