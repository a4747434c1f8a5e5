"""The register budget of the multi-map kernel gf_apply_maps<K, R, NT>
(csrc/maps_kernels.hpp).

maps.hip takes its residency from the w = 8 dispatcher's rule (cap_for,
residency_lds_bytes), which is real only while the kernel fits
kMinWavesPerSimd waves on a SIMD (tests/test_kernel_resources.py).  This
compiles the instantiations of the rebuild shapes -- RS(10,4) with one, two
and four shards lost, RS(12,4) and RS(6,3) with m lost, the widest table
entry -- at both store policies for gfx950 with
-Rpass-analysis=kernel-resource-usage and asserts: no scratch, at least
kMinWavesPerSimd waves per SIMD, and exactly K vector loads in each body --
the per-stripe map index, the pointer tables and the coefficient tables of
the chosen map all stayed scalar loads.
"""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, MAX_WAVES, ROOT, VGPR_FILE, VGPR_GRANULE, _constant, _hipcc

SHAPES = [(10, 1), (10, 2), (10, 4), (12, 4), (6, 3), (16, 4)]  # (K, R)


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{(K, R, NT): {"vgprs", "agprs", "scratch", "occupancy", "vector_loads", ...}} from one device-only compile."""
    d = tmp_path_factory.mktemp("maps_resource_usage")
    lines = ['#include "maps_kernels.hpp"', "namespace ecgpu {", "namespace dev {"]
    for K, R in SHAPES:
        for nt in (1, 3):  # loads nt; stores plain / nt (maps_spec.hip)
            lines.append(f"template __global__ void gf_apply_maps<{K}, {R}, {nt}>(MapsArgs);")
    lines += ["}", "}"]
    src = d / "instantiate.hip"
    src.write_text("\n".join(lines) + "\n")
    cmd = [_hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
           "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "out.s")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*gf_apply_mapsILi(\d+)ELi(\d+)ELi(\d+)EEEv", ln)
        if "Function Name:" in ln:
            cur = tuple(int(x) for x in m.groups()) if m else None
            if cur:
                out[cur] = {}
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"\bAGPRs: (\d+)"),
                         ("sgprs", r"SGPRs: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, ln)
            if m:
                out[cur][key] = int(m.group(1))
    asm = (d / "out.s").read_text()
    for key in out:
        body = re.search(r"^_ZN5ecgpu3dev13gf_apply_mapsILi%dELi%dELi%dEEEvNS0_8MapsArgsE:[^\n]*\n(.*?)s_endpgm"
                         % key, asm, re.S | re.M).group(1)
        out[key].update(v_perm=body.count("v_perm_b32"), v_bitop3=body.count("v_bitop3_b32"),
                        vector_loads=len(re.findall(r"^\s+(?:global|flat|buffer)_load", body, re.M)),
                        dwordx4_loads=len(re.findall(r"^\s+global_load_dwordx4", body, re.M)),
                        readlanes=len(re.findall(r"^\s+v_(?:readlane|writelane)", body, re.M)),
                        scratch_ops=len(re.findall(r"^\s+scratch_", body, re.M)))
    return out


@pytest.mark.parametrize("K,R", SHAPES)
def test_maps_kernels_fit_the_residency_the_dispatcher_assumes(usage, K, R):
    need = _constant("kMinWavesPerSimd")
    for nt in (1, 3):
        u = usage.get((K, R, nt))
        assert u and {"vgprs", "agprs", "scratch", "occupancy"} <= set(u), (K, R, nt, u, sorted(usage))
        by_regs = min(MAX_WAVES, VGPR_FILE // (-(-(u["vgprs"] + u["agprs"]) // VGPR_GRANULE) * VGPR_GRANULE))
        print(f"gf_apply_maps<{K},{R},{nt}>: {u}, {by_regs} waves/SIMD by registers")
        assert u["scratch"] == 0 and u["scratch_ops"] == 0, (K, R, nt, u)
        assert by_regs >= need and u["occupancy"] >= need, (K, R, nt, u, need)
        # the K shard loads are the only vector loads: map index, pointers and tables stay scalar loads
        assert u["dwordx4_loads"] == K and u["vector_loads"] == K, (K, R, nt, u)
        # dense: every coefficient is 3 v_perm per dword
        assert u["v_perm"] == R * K * 4 * 3, (K, R, nt, u)
