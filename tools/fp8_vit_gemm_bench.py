"""W8A8 (fp8 MFMA) vs bf16 GEMM on the block linears of the CLIP and OWL-ViT towers (VSMConfig.vit_w8a8) at the bench's row counts:
FP8_BENCH_CROPS (default 64) crops x 577 CLIP tokens (336 px) / x 2305 OWL-ViT tokens.  Sibling of tools/fp8_gemm_bench.py (the LLaMA
shapes).  Per shape: the kernel the dispatcher picked (vstar_op_gemm_last_tile: 256 = 8-wave, 2564 = 4-wave, 384 = 256^2 + 128-row
tail), mean ms of 10 launches (best of 3 rounds, fp8 and bf16 interleaved) and TFLOP/s.  Real (random) operands, bias everywhere,
residual on out_proj / fc2, quick-GELU on fc1.  The fp8 figures are the GEMM alone: the activation quantisation passes are not in them."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vstar_amd import _lib  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda:0")
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
CROPS = int(os.environ.get("FP8_BENCH_CROPS", "64"))
SHAPES = [("clip qkv", 577, 3072, 1024, 0, False), ("clip out_proj", 577, 1024, 1024, 0, True), ("clip fc1 gelu", 577, 4096, 1024, 1, False),
          ("clip fc2", 577, 1024, 4096, 0, True), ("owl qkv", 2305, 2304, 768, 0, False), ("owl out_proj", 2305, 768, 768, 0, True),
          ("owl fc1 gelu", 2305, 3072, 768, 1, False), ("owl fc2", 2305, 768, 3072, 0, True)]

print(f"{CROPS} crops; kernel source hash {lib.vstar_build_source_hash().decode()}")
print(f"{'shape':14s} {'M':>7s} {'N':>5s} {'K':>5s} | {'fp8 tile':>8s} {'fp8 ms':>8s} {'fp8 TF/s':>9s} | {'bf16 tile':>9s} {'bf16 ms':>8s} {'bf16 TF/s':>9s} | {'bf16/fp8':>8s}")
for name, tokens, N, K, epi, use_res in SHAPES:
    M = CROPS * tokens
    g = torch.Generator(device=dev).manual_seed(N + K)
    a = torch.randn(M, K, generator=g, device=dev).bfloat16()
    w = (torch.randn(N, K, generator=g, device=dev) / K ** 0.5).bfloat16()
    bias = (0.1 * torch.randn(N, generator=g, device=dev)).bfloat16()
    res = torch.randn(M, N, generator=g, device=dev).bfloat16() if use_res else None
    c = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    best8, best16, tile8, tile16 = 1e9, 1e9, 0, 0
    for _ in range(3):
        t = ctypes.c_float(0)
        rc = lib.vstar_op_gemm_fp8(None, P(a), P(w), P(bias), P(res), P(c), M, N, K, epi, 10, ctypes.byref(t))
        assert rc == 0, lib.vstar_last_error(None)
        tile8 = lib.vstar_op_gemm_last_tile()
        best8 = min(best8, t.value)
        run = lambda: lib.vstar_op_gemm(None, P(a), K, P(w), P(bias), P(res), N, P(c), N, 0, M, N, K, epi | _lib.EPI_NOSYNC)  # noqa: E731
        assert run() == 0, lib.vstar_last_error(None)
        tile16 = lib.vstar_op_gemm_last_tile()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            run()
        e1.record()
        torch.cuda.synchronize()
        best16 = min(best16, e0.elapsed_time(e1) / 10)
    fl = 2.0 * M * N * K
    print(f"{name:14s} {M:7d} {N:5d} {K:5d} | {tile8:8d} {best8:8.3f} {fl / best8 / 1e9:9.1f} | {tile16:9d} {best16:8.3f} {fl / best16 / 1e9:9.1f} | {best16 / best8:8.2f}")
    del a, w, res, c
