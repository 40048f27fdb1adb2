"""Provenance of committed evidence: summaries are stamped with a hash of the KERNEL sources, and bench.py only
quotes a PMC figure measured on the kernels it is running.  CPU-only."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_source_hash_is_stable_and_tracks_kernel_edits(tmp_path, monkeypatch):
    from vstar_amd import provenance
    h = provenance.kernel_source_hash()
    assert len(h) == 16 and int(h, 16) >= 0 and h == provenance.kernel_source_hash()
    # a copy of csrc with one kernel byte changed hashes differently; a host-only edit elsewhere does not enter at all
    dst = tmp_path / "csrc"
    shutil.copytree(os.path.join(ROOT, "vstar_amd", "csrc"), dst, ignore=shutil.ignore_patterns("build"))
    monkeypatch.setattr(provenance, "_CSRC", str(dst))
    assert provenance.kernel_source_hash() == h
    with open(dst / "gemm256.hip", "a") as f:
        f.write("\n// edited\n")
    h_edited = provenance.kernel_source_hash()
    assert h_edited != h
    # gemm4w's generated K-loop text is kernel source like any .hip
    with open(dst / "gemm4w_loop.inc", "a") as f:
        f.write("\n// edited\n")
    assert provenance.kernel_source_hash() not in (h, h_edited)


def test_committed_gemm4w_loop_text_is_what_its_generator_emits(tmp_path):
    """vstar_amd/csrc/gemm4w_loop.inc (schedules, register contract) is byte for byte the output of tools/gen_gemm4w_asm.py with its
    schedule switches at their defaults: an edit to either one without the other fails here."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("G4W_")}      # G4W_SHAPE, G4W_SHAPE_PF, G4W_F8_SHAPE, G4W_CPOL, ablations
    out = tmp_path / "gemm4w_loop.inc"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_gemm4w_asm.py"), str(out)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(ROOT, "vstar_amd", "csrc", "gemm4w_loop.inc"), "rb") as f:
        assert out.read_bytes() == f.read()


def test_pmc_summaries_of_this_round_carry_a_stamp():
    """Every r05+ PMC summary under profiles/ is the stamped form ({"kernel_source_hash", "kernels"}); older rounds' files are plain
    lists and are never quoted by bench.py any more."""
    import glob
    for path in glob.glob(os.path.join(ROOT, "profiles", "r0[5-9]_pmc*.json")):
        d = json.load(open(path))
        assert isinstance(d, dict) and len(d["kernel_source_hash"]) == 16 and isinstance(d["kernels"], list), path


def test_power_sampler_parses_rocm_smi_json(tmp_path, monkeypatch):
    """bench.py::_sample_power with a stand-in rocm-smi on PATH: mean power / shader clock over the samples taken while `step` runs."""
    fake = tmp_path / "rocm-smi"
    fake.write_text("#!/bin/sh\necho '{\"card0\": {\"Current Socket Graphics Package Power (W)\": \"1398.0\", "
                    "\"sclk clock speed:\": \"(1737Mhz)\", \"sclk clock level:\": \"1\", \"mclk clock speed:\": \"(2000Mhz)\"}}'\n")
    fake.chmod(0o755)
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "class _T:\n    @staticmethod\n    def synchronize(): pass\n"
            "bench.torch.cuda.synchronize = lambda: None\n"
            "print(__import__('json').dumps(bench._sample_power(lambda: time.sleep(0.05), seconds=0.9)))\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, PATH=str(tmp_path) + os.pathsep + os.environ["PATH"]))
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["power_w"] == 1398.0 and d["sclk_mhz"] == 1737.0 and d["samples"] >= 2


def test_library_carries_the_hash_of_the_sources_it_was_built_from(lib):
    """the stamp identifies the BINARY — build.sh compiles kernel_source_hash() into the library; a tree whose kernel
    sources differ from the loaded library's is refused by checked_hash()."""
    from vstar_amd import provenance
    assert provenance.library_source_hash() == provenance.kernel_source_hash() == provenance.checked_hash()


@pytest.mark.parametrize("dtype_flag", [[], ["--f16"]])
def test_gemm4w_accumulators_are_never_overwritten_before_they_are_read(dtype_flag):
    """gemm4w.hip keeps its accumulators in AGPRs behind the compiler's back (clobbers of the K-loop statement, read back by asm
    statements in the epilogue).  tools/check_gemm4w_agpr.py disassembles the object build.sh links (brought up to date here by
    build.sh's own recipe: seconds when it is) and proves for every kernel that nothing but a read touches an AGPR before the
    epilogue has consumed it (round 6: the register allocator once parked the W piece offsets in a2..a9).  Needs hipcc
    (cross-compiles without a GPU); with hipcc but without its llvm-objdump the checker exits 2 and this test FAILS."""
    import shutil as _sh
    if not (_sh.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "vstar_amd", "csrc")
    b = subprocess.run(["bash", os.path.join(csrc, "build.sh"), "--objects", "gemm4w"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    obj = os.path.join(csrc, "build", "f16_gemm4w.o" if dtype_flag else "gemm4w.o")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_gemm4w_agpr.py"), obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok ") == (12 if dtype_flag else 22)


# One kernel as llvm-objdump -d prints it, cut down to what the rule looks at: the end of the K loop, then the epilogue reading a0..a255
# sixteen at a time (_EPILOGUE_READS).  The two tests below splice ONE compiler-written instruction in between two read statements.
_LOOP_END = """\
	v_mfma_f32_16x16x32_bf16 a[248:251], v[124:127], v[92:95], a[248:251]// 00000000D0A8: D3B580F8 07E2B97C
	s_waitcnt lgkmcnt(0)                                       // 00000000D0B0: BF8CC07F
	v_mfma_f32_16x16x32_bf16 a[252:255], v[124:127], v[92:95], a[252:255]// 00000000D0B4: D3B580FC 07F2B97C
	s_nop 15                                                   // 00000000D0BC: BF80000F
	s_cbranch_scc1 19505                                       // 00000000D0C0: BF854C31 <_ZN7vs_bf1613gemm4w_kernelILi0EEEvNS_10GemmParamsE+0xa1>
	buffer_load_dwordx4 v[4:7], v2, s[8:11], 0 offen           // 00000000D0C4: E05C1000 80020402
"""
_EPILOGUE_READS = ["\tv_accvgpr_read_b32 v%d, a%d                                 // 00000000E3C8: D3D84039 18000100\n" % (57 + n % 16, n)
                   for n in range(256)]
_EPILOGUE_END = """\
	global_store_dwordx4 v[0:1], v[57:60], off                 // 00000000F000: DC7C0000 007F3900
	s_endpgm                                                   // 00000000F008: BF810000
"""


def _check_kernel(spliced, at):
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_gemm4w_agpr", os.path.join(ROOT, "tools", "check_gemm4w_agpr.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    text = _LOOP_END + "".join(_EPILOGUE_READS[:at]) + spliced + "".join(_EPILOGUE_READS[at:]) + _EPILOGUE_END
    consumed, offenders = mod.check_kernel(text.split("\n"))
    return len(consumed), offenders


def test_agpr_rule_reports_an_accumulator_overwritten_before_its_read():
    """The round-6 mis-compile: a VGPR value parked in a40 after only a0..a31 have been read.  Parking in a register whose accumulator
    HAS been consumed (and reading it back) is what the compiler may do, and passes."""
    park = "\tv_accvgpr_write_b32 a%d, v146                             // 00000000E4C8: D3D94028 18000192\n"
    back = "\tv_accvgpr_read_b32 v146, a%d                              // 00000000E4D0: D3D84092 18000128\n"
    assert _check_kernel("", 32) == (256, [])
    assert _check_kernel(park % 3 + back % 3, 32) == (256, [])
    n, offenders = _check_kernel(park % 40, 32)
    assert offenders == ["v_accvgpr_write_b32 a40, v146"]
    assert n == 255                        # the read of a40 that follows returns the parked value: not a consumed accumulator


def test_agpr_rule_reports_a_load_into_an_agpr():
    """On gfx950 a load can have an AGPR destination: anything that names an AGPR in the window and is neither of the two accvgpr
    forms is a violation — also in a register that is already consumed, also as a source, also v_accvgpr_mov."""
    for bad in ("global_load_dword a40, v[2:3], off", "ds_read_b128 a[4:7], v9 offset:2048", "scratch_store_dword off, a200, s32",
                "v_accvgpr_mov_b32 a3, a2"):
        n, offenders = _check_kernel("\t%s                     // 00000000E4C8: DC508000 287F0002\n" % bad, 32)
        assert offenders == [bad], bad
    # an MFMA behind the first reads moves the window's start behind it: the reads before it no longer count as consumed
    n, _ = _check_kernel("\tv_mfma_f32_16x16x32_bf16 a[0:3], v[4:7], v[8:11], a[0:3]   // 00000000E4C8: D3B580FC 07F2B97C\n", 32)
    assert n == 256 - 32
