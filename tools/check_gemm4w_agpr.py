#!/usr/bin/env python
"""Proves, on the code object that SHIPS, that nothing but gemm4w's hand-written statements touches the AGPRs while they hold the
accumulators (round 6).  gemm4w.hip keeps a 128 x 128 fp32 tile per wave in a0..a255 across the K-loop asm statement and reads it back
with v_accvgpr_read statements in the epilogue; the register allocator does not know that and, under pressure, parks VGPR values in
AGPRs.  Every epilogue read statement clobbers the whole AGPR file, so no compiler value can live in an AGPR ACROSS a read; what is
left is short-term parking between two reads, and that is harmless exactly when the AGPR has already been consumed.

The script takes the objects build.sh made (build/gemm4w.o, build/f16_gemm4w.o: it compiles nothing and knows no flags), extracts
their gfx950 code object and disassembles it with the llvm-objdump that sits beside hipcc's clang.  For every gemm4w kernel, from the
LAST MFMA to the end of the kernel, EVERY instruction that names an AGPR in any operand position must be
  * a v_accvgpr_read_b32 (an epilogue statement consuming an accumulator, or the compiler reading back what it parked), or
  * a v_accvgpr_write_b32 to a register that has already been consumed;
anything else — a load, store, LDS or scratch instruction with an AGPR operand, v_accvgpr_mov, an MFMA — is a violation, and all
256 accumulators must be consumed.  build.sh runs it before the link; tests/test_provenance.py runs it and tests the rule itself.
usage: python tools/check_gemm4w_agpr.py OBJECT...   exit code 1 and a report on violation, 2 if there is no llvm-objdump"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

# {NONE, QUICK_GELU, RELU, SILU_MUL} x {plain, prefetch} x {whole tiles, ragged last row tile} (+ eight W8A8 and four block-scaled W8A8
# kernels in the bf16 build); gemm4w_vit8.o: the W8A8 quick-GELU kernels (ViT fc1) x {plain, prefetch, ragged}
KERNELS = {"gemm4w.o": 22, "f16_gemm4w.o": 12, "gemm4w_vit8.o": 3}
NAMES_AGPR = re.compile(r"\ba(\d+\b|\[)")


def find_objdump():
    """The llvm-objdump of the compiler that built the objects: beside the clang that hipcc runs (`hipcc --version`: InstalledDir)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        m = re.search(r"^InstalledDir: (.+)$", subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout, re.M)
    except OSError:
        m = None
    path = os.path.join(m.group(1).strip(), "llvm-objdump") if m else ""
    return path if os.path.isfile(path) else None


def disassemble(objdump, obj):
    """Instruction lines of every gemm4w kernel of the object's gfx950 code object: {symbol: [text, ...]}."""
    with tempfile.TemporaryDirectory() as td:        # (--offloading writes the extracted images next to the file it reads: a copy)
        shutil.copy(obj, os.path.join(td, "obj.o"))
        subprocess.check_call([objdump, "--offloading", "obj.o"], cwd=td, stdout=subprocess.DEVNULL)
        images = glob.glob(os.path.join(td, "*gfx950*"))
        assert len(images) == 1, f"{obj}: expected one gfx950 code object, found {[os.path.basename(x) for x in images]}"
        text = subprocess.run([objdump, "-d", images[0]], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = kernels.setdefault(m.group(1), []) if "gemm4w_kernel" in m.group(1) else None
        elif cur is not None and line.strip():
            cur.append(line)
    return kernels


def check_kernel(lines):
    """The rule on one kernel's disassembly -> (accumulators consumed, violating instructions)."""
    ins = [re.sub(r"<[^>]*>", "", x.split("//")[0]).strip() for x in lines]          # (no encoding bytes, no branch-target symbols)
    last_mfma = max((i for i, x in enumerate(ins) if x.startswith("v_mfma")), default=-1)
    consumed, parked, offenders = set(), set(), []
    for x in ins[last_mfma + 1:]:
        if not NAMES_AGPR.search(x):
            continue
        rd = re.fullmatch(r"v_accvgpr_read_b32 v\d+, a(\d+)", x)
        wr = re.fullmatch(r"v_accvgpr_write_b32 a(\d+), \S+", x)
        if rd:
            n = int(rd.group(1))
            if n in parked:
                parked.discard(n)            # the compiler reading back what it parked
            else:
                consumed.add(n)              # an epilogue read statement: the accumulator is consumed
        elif wr:
            n = int(wr.group(1))
            if n not in consumed:
                offenders.append(x)          # overwrites an accumulator the epilogue has not read yet
            parked.add(n)
        else:
            offenders.append(x)
    return consumed, offenders


def main(objects):
    objdump = find_objdump()
    if objdump is None:
        print("gemm4w AGPR check: no llvm-objdump beside the clang of " + os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
        return 2
    bad = 0
    for obj in objects:
        kernels = disassemble(objdump, obj)
        want = KERNELS[os.path.basename(obj)]
        assert len(kernels) == want, f"{obj}: expected {want} gemm4w kernels, found {len(kernels)}"
        for name, lines in kernels.items():
            consumed, offenders = check_kernel(lines)
            ok = not offenders and len(consumed) == 256
            print(("ok   " if ok else "FAIL ") + name[-44:], "accumulators consumed", len(consumed), "violations", len(offenders), offenders[:4])
            bad += not ok
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
