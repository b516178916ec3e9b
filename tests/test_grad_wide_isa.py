"""ISA guards on the wide gradient-stage kernels (grad_wide_kernels.hpp), from the built gfx950 code object: no scratch
traffic anywhere in them (their inner loops hold 4 x 4 register tiles; a spill there would reload on every dimension
step), and the scan's distance is the same add / fused multiply-add chain as knn_kernel's, so both scans see the same
distances and order ties alike."""
import os
import re
import subprocess

import pytest

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNELS = {
    "knn_wide_kernel": "_ZN6corrla1k15knn_wide_kernelENS0_12WideScanArgsE",
    "grad_fit_wide_kernel": "_ZN6corrla1k20grad_fit_wide_kernelENS0_11WideFitArgsE",
    "knn_kernel": "_ZN6corrla1k10knn_kernelEPKdlliS2_liPi",
}


@pytest.fixture(scope="module")
def disasm(tmp_path_factory):
    from corrla_rs_amd import build as B
    lib = B.build_product()
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    data = open(lib, "rb").read()
    tmp = tmp_path_factory.mktemp("isa") / "device_code_object.o"
    out = {}
    for mm in re.finditer(b"\x7fELF", data):
        i = mm.start()
        if data[i + 18: i + 20] == b"\xe0\x00":      # e_machine = EM_AMDGPU
            tmp.write_bytes(data[i:])
            for name, sym in KERNELS.items():
                text = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", "--disassemble-symbols=" + sym, str(tmp)],
                                      capture_output=True, text=True).stdout
                out[name] = out.get(name, []) + [l for l in text.splitlines() if "\t" in l]
    return out


@pytest.mark.parametrize("name", ["knn_wide_kernel", "grad_fit_wide_kernel"])
def test_wide_kernels_keep_clear_of_scratch(disasm, name):
    lines = disasm[name]
    assert len(lines) > 500, "%s not found in the device code" % name
    bad = [l.strip() for l in lines if "scratch_" in l]
    assert not bad, bad[:4]


def test_wide_scan_distance_chain_matches_knn_kernel(disasm):
    def mix(lines):
        return {op: sum(op in l for l in lines) for op in ("v_fmac_f64", "v_fma_f64", "v_mul_f64", "v_add_f64")}
    wide, ref = mix(disasm["knn_wide_kernel"]), mix(disasm["knn_kernel"])
    # the 4 x 4 tile: 16 subtractions and 16 accumulations per dimension step, fused in both kernels
    assert wide["v_fmac_f64"] + wide["v_fma_f64"] >= 16 and wide["v_add_f64"] >= 16, wide
    assert ref["v_fmac_f64"] + ref["v_fma_f64"] > 0 and wide["v_mul_f64"] == 0 and ref["v_mul_f64"] == 0, (wide, ref)
