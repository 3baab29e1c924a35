// The one fp32 implicit-GEMM tile of the inference convolutions (conv_f32.hip, resnet_f32.hip; sagan_f32.hip's first-layer GEMM is a
// sixth entry on it), on the f32-input matrix instruction
// (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain, at 1/16 of the bf16 MFMA rate): its constants, what the hosts of
// its five entries decide alike, and this description.  The device text is conv_f32_tile_body.inc, included inside each kernel.
//
// Implicit GEMM: M rows (pixels), N = Co, K = taps x Cip (Cip = Ci, or 4 for the 3-channel stem).  A workgroup of four waves owns
// one BM x BN output tile and walks ALL of its K in steps of 16: no split-K, no atomics, no inter-workgroup state.
//   A tile  gathered from NHWC fp32, 16 bytes (4 channels of one tap) per load; what a row reads for a tap is its kernel's Gather;
//           rows beyond M and k beyond the real K are zeros
//   B tile  rows of the packed weights [Co][Kp] (k contiguous, zero-filled to Kp = ceil16(K)); rows beyond Co are zeros
//   LDS     As[row][16 + 4], Bs[col][16 + 4] floats, two stages (40 KB for the largest tile).  A lane reads its row's k-half
//           (4 floats at 8 g + 4 (lane >> 5)) with one ds_read_b128; the row stride of 20 dwords puts the 16 lanes of every
//           ds_read_b128 lane group on 16 distinct 4-bank spans of the 64 banks
//   MFMA    32x32x2: lane l supplies A[row l & 31][k half l >> 5] and B[k half l >> 5][col l & 31], so instruction e of half-step
//           g multiplies k = 8 g + e and 8 g + 4 + e.  The order of K is the same for every tile shape, every pixel, every batch,
//           every entry: there is one k loop, the one below.
//   C       col = lane & 31 (a channel: 32 lanes store 128 contiguous bytes), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5);
//           z = fmaf(acc, scale, shift) goes to the kernel's Store
// The next step's global loads are issued into registers before the current step's MFMAs and stored to the other LDS stage behind
// them: one barrier per step.
// Why the body is text and not a function template with policy objects: every instantiation compiles to the instruction stream
// it had when the tile stood three times in the sources (docs/lab_notebook.md, round 16).  A policy object holding `const Args&`
// cost the epilogue its unswitched activation branches, one holding a copy moved the kernel-argument loads, a load-and-zero
// helper turned the pad-channel zero into a select that waits for the prefetch in every k step, and lambdas came close but not
// there: a callee is simplified alone before it is inlined.  After any change here, compare the assembly with the last release's.
#pragma once
#include "common.hpp"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
constexpr int CF_BK = 16, CF_LDK = CF_BK + 4, CF_THREADS = 256;

// ---- what the hosts of the five entries decide alike ------------------------------------------------------------------------
inline int cf_cip(int Ci) { return Ci == 3 ? 4 : Ci; }
// the row stride of the packed weights: `taps` taps of cf_cip(Ci) channels, zero-filled to a whole k step
inline int cf_kp(int Ci, long long taps) { return (int)((taps * cf_cip(Ci) + CF_BK - 1) / CF_BK * CF_BK); }

// the tile of M rows x Co channels (0: 128 x 128, 1: 64 x 64, 2: 128 x 32)
inline int cf_tile(long long M, int Co) {
    if (Co <= 32) return 2;
    const long long big = ((M + 127) / 128) * ((Co + 127) / 128);
    return (Co >= 128 && big >= 256) ? 0 : 1;              // 128 x 128 tiles once they fill the chip, else 64 x 64
}

// what every entry refuses alike, the kernel's shape aside; 0 when there is nothing to refuse
inline int cf_common(const gcc_conv_t* c, int pad_h, int pad_w, int dilation) {
    if (!c || c->N <= 0 || c->H <= 0 || c->W <= 0 || c->Ci <= 0 || c->Co <= 0 || c->KH <= 0 || c->KW <= 0 || c->stride <= 0 ||
        pad_h < 0 || pad_w < 0 || dilation < 1)
        return GCC_ERR_BAD_ARG;
    if (c->ldx <= 0 || c->ldy <= 0 || c->xoff < 0 || c->yoff < 0 || (c->ldx & 3) || (c->xoff & 3) || (c->ldy & 3) || (c->yoff & 3))
        return GCC_ERR_BAD_ARG;
    return 0;
}

// the launch of tile `route` (cf_tile) of a kernel whose Args hold M and Co; z: the grid's third side (the phases)
template <class Args>
void cf_launch_tile(void (*k128)(Args), void (*k64)(Args), void (*k128x32)(Args), const Args& a, unsigned z, int route, hipStream_t st) {
    if (route == 0) hipLaunchKernelGGL(k128, dim3(cdiv(a.M, 128), cdiv(a.Co, 128), z), dim3(CF_THREADS), 0, st, a);
    else if (route == 1) hipLaunchKernelGGL(k64, dim3(cdiv(a.M, 64), cdiv(a.Co, 64), z), dim3(CF_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k128x32, dim3(cdiv(a.M, 128), 1, z), dim3(CF_THREADS), 0, st, a);
}
// KERNEL<MI, NI, WM, WN, FLAG>: a function template has no other way into a call than its name
#define CF_LAUNCH_TILE(KERNEL, FLAG, a, z, route, st) \
    cf_launch_tile(KERNEL<2, 2, 2, 2, FLAG>, KERNEL<1, 1, 2, 2, FLAG>, KERNEL<1, 1, 4, 1, FLAG>, a, z, route, st)

}  // namespace
