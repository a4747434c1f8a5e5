"""The register budget the w = 8 dispatcher's residency rule relies on.

dispatch_w8.hip caps resident workgroups per CU with an unused dynamic LDS
allocation (residency_lds_bytes: at most kCapMaxBlocks per CU).  A 256-thread
workgroup puts one wave on each SIMD, so a cap of N workgroups per CU is real
only while the kernel's VGPR allocation lets N waves share a SIMD; a kernel
that needs more registers runs at its register limit whatever the dispatcher
asks for, and a launch left uncapped "for the occupancy" gets no more than
that limit either.  This compiles the production instantiations of the
bench's timed encode and of the C4 / C5 launches (both store policies) for
gfx950 with -Rpass-analysis=kernel-resource-usage and asserts: no scratch,
and at least kMinWavesPerSimd waves per SIMD -- the constant the dispatcher
states, which must cover kCapMaxBlocks.  It also holds the RS(10,4) encode to
its v_perm / v_bitop3 counts and every kernel to K vector loads (the pointer
and coefficient tables stay scalar loads).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "erasure_coding_test_amd", "csrc")

# (K, R, UnitMask): C3 encode (timed), C5 encode, C4 decode{0,1,2,3}, C2 encode, the widest table entry
SHAPES = [(10, 4, 3), (12, 4, 3), (10, 4, 0), (6, 3, 3), (16, 4, 0), (16, 3, 0)]
VGPR_FILE = 512     # per SIMD lane on gfx950 (unified VGPR + AGPR file)
VGPR_GRANULE = 8
MAX_WAVES = 8


def _constant(name):
    src = open(os.path.join(CSRC, "dispatch_w8.hip")).read()
    m = re.search(r"constexpr int %s = (\d+);" % name, src)
    assert m, f"dispatch_w8.hip no longer defines {name}"
    return int(m.group(1))


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{(K, R, U, NT): {"vgprs", "agprs", "scratch", "occupancy"}} from one device-only compile."""
    d = tmp_path_factory.mktemp("resource_usage")
    lines = ['#include "gf_kernels.hpp"', "namespace ecgpu {", "namespace dev {"]
    for K, R, U in SHAPES:
        for nt in (1, 3):  # loads nt; stores plain / nt (gf_spec.hip apply_fn)
            lines.append(f"template __global__ void gf_apply<{K}, {R}, {U}, {nt}>(ApplyArgs);")
    lines += ["}", "}"]
    src = d / "instantiate.hip"
    src.write_text("\n".join(lines) + "\n")
    cmd = [_hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
           "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "out.s")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*gf_applyILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEEv", ln)
        if "Function Name:" in ln:
            cur = tuple(int(x) for x in m.groups()) if m else None
            if cur:
                out[cur] = {}
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"\bAGPRs: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, ln)
            if m:
                out[cur][key] = int(m.group(1))
    asm = (d / "out.s").read_text()
    for key in out:
        K, R, U, nt = key
        body = re.search(r"^_ZN5ecgpu3dev8gf_applyILi%dELi%dELi%dELi%dEEEvNS0_9ApplyArgsE:[^\n]*\n(.*?)s_endpgm"
                         % key, asm, re.S | re.M).group(1)
        out[key].update(v_perm=body.count("v_perm_b32"), v_bitop3=body.count("v_bitop3_b32"),
                        vector_loads=len(re.findall(r"^\s+(?:global|flat|buffer)_load", body, re.M)),
                        scratch_ops=len(re.findall(r"^\s+scratch_", body, re.M)))
    return out


def test_dispatch_constants_are_consistent():
    assert _constant("kMinWavesPerSimd") >= _constant("kCapMaxBlocks") >= 3


@pytest.mark.parametrize("K,R,U", SHAPES)
def test_production_kernels_fit_the_residency_the_dispatcher_assumes(usage, K, R, U):
    need = _constant("kMinWavesPerSimd")
    for nt in (1, 3):
        u = usage.get((K, R, U, nt))
        assert u and {"vgprs", "agprs", "scratch", "occupancy"} <= set(u), (K, R, U, nt, u, sorted(usage))
        by_regs = min(MAX_WAVES, VGPR_FILE // (-(-(u["vgprs"] + u["agprs"]) // VGPR_GRANULE) * VGPR_GRANULE))
        print(f"gf_apply<{K},{R},{U},{nt}>: {u}, {by_regs} waves/SIMD by registers")
        assert u["scratch"] == 0, (K, R, U, nt, u)
        assert by_regs >= need and u["occupancy"] >= need, (K, R, U, nt, u, need)
        # the K shard loads are the only vector loads: pointers and 3-bit-slice tables stay scalar loads
        assert u["vector_loads"] == K and u["scratch_ops"] == 0, (K, R, U, nt, u)


def test_encode_keeps_its_operation_counts(usage):
    """RS(10,4) encode: 27 multiply terms x 4 dwords x 3 v_perm, and XOR3 folding two terms at a time."""
    for nt in (1, 3):
        u = usage[(10, 4, 3, nt)]
        assert (u["v_perm"], u["v_bitop3"]) == (324, 188), u
