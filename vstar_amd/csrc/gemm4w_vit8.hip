// gemm4w_vit8.hip — the W8A8 quick-GELU instantiations of the 4-wave kernel (fc1 of the CLIP / OWL-ViT towers, vit_w8a8): gemm4w.hip
// compiled a second time with only gemm4w_gelu8_lp public.  An object of their own so that each object's kernel count stays what
// tools/check_gemm4w_agpr.py (and the test that runs it on gemm4w.o) expects; same templates, same K-loop texts, same epilogue.
// bf16 library only (the fp8 operands exist there only).
#ifdef VSTAR_LP_F16
#error "gemm4w_vit8.hip: bf16 library only"
#endif
#undef G4W_TIMELINE
#define G4W_TU_VIT8
#pragma clang diagnostic ignored "-Wunused-function"
#include "gemm4w.hip"
