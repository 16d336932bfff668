// Compile-time configuration of the kernels, in one place.
//
// 1. Instrumentation: ONE enable macro, VIHMC_DIAG (default 0 = the product build). A variant build sets it on the
//    hipcc line (make -C vi-hmc_amd OUT=$PWD/_ab/<v>.so BUILD=$PWD/build/<v> EXTRA=-DVIHMC_DIAG=<value>); its fields
//    select in-kernel phase stamps (s_memtime per phase into a __device__ array of their own, read back by
//    profiles/scripts/diag/stamps_*.py). The results stay right, the timing is perturbed. vihmc_version() reports
//    the value ("diag=<n>"); plan creation and vihmc._lib refuse a library with VIHMC_DIAG != 0 unless
//    VIHMC_ALLOW_DIAG=1 (the stamp readers only). Every other bit is an error: bits 0-3 and 10-16 selected
//    timing-only ablations (wrong results by design) until those were removed, and such a build line must not
//    silently build the product.
//
//    field (bits)         name            meaning
//    4                    FWD_STAMP       per-layer phase stamps of k_fwd_fused_bf (stamps_fwd.py)
//    5                    BB_STAMP        per-sub-tile stamps of k_bwd_bf2 (stamps_bwd.py)
//    6                    CH_STAMP        per-layer stamps of k_bwd_chain (stamps_chain.py)
//    7-8                  CB_STAMP        side-A contraction stamps, two placements 1 / 2 (stamps_side_a.py)
//    9                    GR_STAMP        per-block stamps of k_gram_a's T_b units (stamps_gram.py)
//
// 2. Tuning constants of the shipped kernels (not switches: an A/B edits this header and builds into _ab/).
#pragma once

#ifndef VIHMC_DIAG
#define VIHMC_DIAG 0
#endif
#if (VIHMC_DIAG) & ~0x3F0
#error "VIHMC_DIAG: only the stamp fields (bits 4-9) exist; the timing-only ablation fields were removed"
#endif

#define VIHMC_DIAG_FIELD(shift, bits) ((VIHMC_DIAG >> (shift)) & ((1 << (bits)) - 1))
#define FWD_STAMP VIHMC_DIAG_FIELD(4, 1)
#define BB_STAMP VIHMC_DIAG_FIELD(5, 1)
#define CH_STAMP VIHMC_DIAG_FIELD(6, 1)
#define CB_STAMP VIHMC_DIAG_FIELD(7, 2)
#define GR_STAMP VIHMC_DIAG_FIELD(9, 1)

// waves per workgroup of the bf16x6 forward (16 rows each): 12 = 3 per SIMD at 168 VGPRs
#define FWD_BF_NW 12
// slab count from which a reduce block's four waves split the slabs (k_reduce)
#define REDUCE_GROUP_MIN 32
// gradient-gather K slices per chain at most (launch_gather_prior picks ~256 blocks over all chains)
#define GATHER_SPLIT_N 256
// Gram form, centred: cost of a two-chain T_t unit (k_gram_b2) in one-chain units, for launch_gram's row-group split
#define GRAM_B2_RATIO 1.7
// centred Gram form, 8+ chains: Gram-t slabs per T_b slab (k_gram_a's Gram-t units GRAM_T_SPLIT times shorter)
#define GRAM_T_SPLIT 2
