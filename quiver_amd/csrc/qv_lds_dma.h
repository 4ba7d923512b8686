// qv_lds_dma.h — rows from global memory straight into LDS (global_load_lds_*: no register in between) and the explicit wait that goes with
// them.  Shared by the kernels that keep their query operands in registers and stream rows through an LDS ring (qv_qreg.hip, qv_int8.hip).
// The requests are inline assembly: the compiler would otherwise order EVERY LDS read behind the youngest LDS-DMA (vmcnt(0): it cannot tell
// the ring's stages apart).  Requests complete in order per wave, so s_waitcnt vmcnt(N) certifies all but the wave's N youngest.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace qv {

typedef __attribute__((address_space(3))) unsigned char qlds_u8;

template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// one 1-KiB request: lane l moves the 16 bytes at src + voff(l) + OFF to LDS byte lds_byte_addr + OFF + 16 l; src is wave-uniform.
// (The same request through a buffer descriptor — base in the descriptor, the piece's offset in a scalar register — measures the same:
// 518 / 393 us against 517 / 388 in k_qreg_filter; what a request costs the issuing wave, ~55 ns, is not its address arithmetic.)
template <int OFF>
__device__ __forceinline__ void dma_piece(const void* src, uint32_t voff, uint32_t lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %2\n\t"
                 "s_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:%3 nt"
                 :: "v"(voff), "s"(src), "s"(lds_byte_addr), "n"(OFF) : "memory");   // (m0 is written; the compiler keeps nothing in it across statements in these kernels: no movrel, GWS or LDS-DMA builtins)
}

// 256 bytes, one dword per lane (byte offset voff from the wave-uniform src), to lds_byte_addr + 4 lane: the row constants of a tile
__device__ __forceinline__ void dma_words(const void* src, uint32_t voff, uint32_t lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %2\n\t"
                 "s_nop 0\n\t"
                 "global_load_lds_dword %0, %1"
                 :: "v"(voff), "s"(src), "s"(lds_byte_addr) : "memory");
}

}  // namespace qv
