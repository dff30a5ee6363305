// Device helpers shared by the tile kernels of libfgcn (gfx950 only): buffer descriptors, the workgroup order over the XCDs, the
// transposing LDS read, compile-time slot loops and the split adjacency planes.  Moving a kernel's local helper here must leave its
// instructions unchanged: tools/kdiff.py compares the device code of every source with another revision's.
#pragma once
#include <utility>

#include "fgcn_common.hpp"

namespace fgcn {

// Buffer descriptor of `bytes` bytes at `ptr` (raw 32-bit offsets; a load past the end returns 0, a store is dropped).  Three sites
// call the builtin themselves with BUFFER_FLAGS (the gated-addend descriptors of fgcn_spatial_bwd_tile.hip, the bias descriptor of
// emb_wgrad_tile_kernel): through this function the compiler places the descriptor earlier and allocates other scalar registers.
constexpr int BUFFER_FLAGS = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* ptr, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, bytes, BUFFER_FLAGS);
}

// Tile of workgroup b when consecutive workgroups go round the 8 XCDs: every XCD walks its own run of `per_xcd` consecutive tiles
// (neighbouring tiles share operands in that XCD's L2)
__device__ __forceinline__ int xcd_tile(unsigned b, int per_xcd) { return (b & 7) * per_xcd + (b >> 3); }

// ds_read_b64_tr_b16: the lane's four 16-bit values of a 16 x 16 block read across its rows (the operand fragment of a product with
// the block's transpose)
__device__ __forceinline__ u32x2 lds_read_tr16(const unsigned char* p) {
    using v4s = __attribute__((ext_vector_type(4))) short;
    const v4s v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p));
    return __builtin_bit_cast(u32x2, v);
}

// fn(std::integral_constant<int, S>{}) for every S of the sequence: a slot loop as straight-line code with compile-time slot indices
template <class Fn, int... S>
__device__ __forceinline__ void for_slots(Fn&& fn, std::integer_sequence<int, S...>) {
    (fn(std::integral_constant<int, S>{}), ...);
}

// Split 32 x 32 matrices in LDS / the dx workspace: planes [matrix][part slot][32 rows][AHB bytes] of bf16, one value per
// (row, column); AHB = 32 columns x bf16 + 16 bytes of padding (conflict-free b128 reads)
constexpr int AHB = 80;

// one value -> its NP bf16 parts at (row, col) of matrix m (LP part slots per matrix: 3, or NP where a one-part layout is packed)
template <int NP, int LP = 3>
__device__ __forceinline__ void put_split(unsigned char* planes, int m, int row, int col, float value) {
    unsigned ph, pm, pl;
    split_bf16_pair(value, 0.f, ph, pm, pl);
    unsigned short* d = reinterpret_cast<unsigned short*>(planes + ((m * LP) * 32 + row) * AHB) + col;
    d[0] = (unsigned short)ph;
    if constexpr (NP == 3) {
        d[32 * AHB / 2] = (unsigned short)pm;
        d[2 * 32 * AHB / 2] = (unsigned short)pl;
    }
}

// The three adjacency matrices src[k][v][w] (V x V floats each; joints from V on read as 0) of one sample, split
// once per workgroup into planes[k][part][row][col]: row = w, col = v (one ds_read_b128 = the 8 joints v of a lane's fragment), or
// ROW_IS_V: row = v, col = w
template <int NP, int NTHREADS, bool ROW_IS_V>
__device__ __forceinline__ void stage_adjacency_planes(unsigned char* planes, const float* src, int V, int tid) {
    for (int i = tid; i < 3 * 32 * 32; i += NTHREADS) {
        const int k = i >> 10, hi = (i >> 5) & 31, lo = i & 31;
        const int v = ROW_IS_V ? hi : lo, w = ROW_IS_V ? lo : hi;
        const float a = (v < V && w < V) ? src[(k * V + v) * V + w] : 0.f;
        put_split<NP>(planes, k, hi, lo, a);
    }
}

}  // namespace fgcn
