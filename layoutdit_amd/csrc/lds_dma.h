// LDS-DMA (global_load_lds_dwordx4): one instruction moves 64 lanes x 16 B = 1 KB from global memory straight into LDS - no
// registers, no scatter writes.  The LDS destination is wave-uniform (it travels in M0); lane l's 16 bytes land at offset 16 l.
// The one definition of the pieces the GEMM and attention kernels stage their operands with.
#pragma once
#include <hip/hip_runtime.h>

namespace ldit {

// A piece from a per-lane 64-bit address, through the builtin.  hipcc sees it: LDS reads that may alias a piece in flight are
// guarded with s_waitcnt vmcnt(0).
__device__ __forceinline__ void glds16(const void *gsrc, char *lds_wave_base)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                     (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

// A piece with a wave-uniform 64-bit base in SGPRs and a per-lane 32-bit BYTE offset: `global_load_lds_dwordx4 voff, s[base]`.
// The builtin only takes a per-lane 64-bit pointer: two or three VALU instructions per piece (offset + k, widen, add) and a live
// VGPR pair; here the advance along the operand lives in the scalar base and the lane offset is a constant of the kernel.
// M0 (the LDS destination) is compiler-reserved: saved and restored inside the statement (cdna guide 5.7).  Invisible to hipcc's
// waitcnt pass: every consumer of the staged data sits behind an explicit s_waitcnt vmcnt.  hipcc pads no hazards inside an asm
// statement either: the base must not come fresh out of a v_readfirstlane (five wait states, scripts/audit_dma_hazard.py).
__device__ __forceinline__ void glds16_sbase(const void *ubase, unsigned voff_bytes, unsigned lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff_bytes), "s"(ubase), "s"(lds_dst)
                 : "memory");
}

// The same piece from a per-lane 64-bit address (ragged tiles, zero-page redirects), also as an asm statement: a kernel whose every
// LDS-DMA is invisible to hipcc keeps its LDS reads free of the vmcnt(0) guards hipcc puts in front of reads that may alias a
// builtin LDS-DMA in flight.  `lds_dst` must be wave-uniform (it travels in M0).
__device__ __forceinline__ void glds16_vaddr(const void *gsrc, unsigned lds_dst)
{
    unsigned keep;
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(dst)
                 : "memory");
}

}  // namespace ldit
