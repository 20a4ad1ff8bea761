// vdjx_scan.h -- the exclusive prefix sum of the device code: every stage that turns counts into offsets calls one of the two forms.
//
//   out[i] = f(in[0]) + ... + f(in[i - 1])   for i = 0 .. n: out holds n + 1 elements, out[n] is the total, n == 0 writes out[0] = 0.
//
// `in` and `out` do not alias; n < 2^31.  T (the type of out: u32 or u64) and In are taken from the pointers; f is applied to every
// element as it is loaded (identity by default; vdjx_quant.hip passes q_deg_key).  Sums wrap in T.  Everything here has internal
// linkage (the anonymous namespace): every translation unit that includes the header gets kernels of its own.
//
//   vdjx_scan_one   one launch, one workgroup: counts of up to a few million (bucket, slice and block counts)
//   vdjx_scan_wide  three launches over the whole device: per-record and per-class counts
// The test suite reaches both through vdjx_scan_u32 (include/vdjx.h; defined in vdjx_rindex.hip, one of the files that include this).
#pragma once

#include "vdjx_common.h"

#define VDJX_SCAN_TILE_U32 8192u      // elements per tile of the one-launch form, 4-byte sums
#define VDJX_SCAN_TILE_U64 8192u      // ... 8-byte sums (66 KB of LDS)
#define VDJX_SCAN_BLOCK 4096u         // elements per workgroup of the device-wide form, every caller

namespace {

struct vdjx_scan_identity {
	template <typename X> __device__ X operator()(X x) const { return x; }
};

template <typename T> __host__ __device__ constexpr u32 vdjx_scan_tile() { return sizeof(T) == 8 ? VDJX_SCAN_TILE_U64 : VDJX_SCAN_TILE_U32; }

// wave-wide inclusive prefix sums of either width (vdjx_common.h; all 64 lanes active)
__device__ inline u32 vdjx_scan_wave(u32 v) { return (u32) vdjx_wave_scan_add((int) v); }
__device__ inline u64 vdjx_scan_wave(u64 v) { return vdjx_wave_scan_add(v); }

// for kernels that scan as a step of other work (k_plan, k_seg_offsets): the exclusive prefix of one value per thread over the
// workgroup and the total, in every thread (all call it; whole waves, at most 1024 threads; tmp: 16 elements of LDS)
template <typename T> __device__ inline T vdjx_block_scan(T v, T* tmp, T& total) {
	const T incl = vdjx_scan_wave(v);
	__syncthreads();
	if ((threadIdx.x & 63u) == 63u) tmp[threadIdx.x >> 6] = incl;
	__syncthreads();
	T base = 0, tot = 0;
	for (u32 w = 0; w < blockDim.x / 64; w++) { const T x = tmp[w]; if (w < (threadIdx.x >> 6)) base += x; tot += x; }
	total = tot;
	return base + incl - v;
}

// ---- the one-launch form: one 1024-thread workgroup ---------------------------------------------------------------------------------
// Tiles of 8,192 elements go through LDS: read and written with consecutive lanes on consecutive addresses, summed eight per thread from
// a padded layout (index i at i + i/32: the 32 lanes of a half-wave on 32 banks), a carry from tile to tile.  Inside a tile: DPP prefix
// sums inside the waves, then the totals of the waves before one's own -- three barriers instead of the twenty of a 1,024-wide
// Hillis-Steele scan in LDS.
// (Measured, and why no thread walks a run of its own in global memory: a thread reading its own 32 consecutive counters made 2^15
// counters a chain of 32 dependent line fills, 52 us at 10 M pairs between the histogram and the partition of the k-mer build; one
// workgroup of that kind over the 32,768 block counts of a 10 M-pair pool's read-index table was 56 us.)
template <typename In, typename T, typename F>
__global__ __launch_bounds__(1024) void k_scan_one(const In* __restrict__ in, u32 n, T* __restrict__ out, F f) {
	constexpr u32 TILE = vdjx_scan_tile<T>(), PER = TILE / 1024u;
	static_assert(TILE % 1024u == 0 && 32u % PER == 0, "a thread's PER elements lie inside one padded group of 32");
	__shared__ T buf[TILE + TILE / 32];
	__shared__ T wsum[16];
	__shared__ T s_carry;
	const u32 t = threadIdx.x, lane = t & 63u, wv = t >> 6;
	if (t == 0) s_carry = 0;
	__syncthreads();
	for (u32 base = 0; base < n; base += TILE) {
#pragma unroll
		for (u32 j = 0; j < PER; j++) {
			const u32 i = j * 1024u + t;
			buf[i + (i >> 5)] = base + i < n ? (T) f(in[base + i]) : (T) 0;
		}
		__syncthreads();
		T v[PER], sum = 0;
#pragma unroll
		for (u32 e = 0; e < PER; e++) { const u32 i = PER * t + e; v[e] = buf[i + (i >> 5)]; sum += v[e]; }
		const T incl = vdjx_scan_wave(sum);
		if (lane == 63) wsum[wv] = incl;
		__syncthreads();
		T run = s_carry + incl - sum;
		for (u32 w = 0; w < wv; w++) run += wsum[w];
#pragma unroll
		for (u32 e = 0; e < PER; e++) { const u32 i = PER * t + e; buf[i + (i >> 5)] = run; run += v[e]; }
		__syncthreads();
#pragma unroll
		for (u32 j = 0; j < PER; j++) {
			const u32 i = j * 1024u + t;
			if (base + i < n) out[base + i] = buf[i + (i >> 5)];
		}
		if (t == 1023) s_carry = run;                         // (thread 1023's running sum is the tile's end)
		__syncthreads();
	}
	if (t == 0) out[n] = s_carry;
}

template <typename In, typename T, typename F = vdjx_scan_identity>
inline void vdjx_scan_one(hipStream_t st, const In* in, u32 n, T* out, F f = F()) {
	hipLaunchKernelGGL((k_scan_one<In, T, F>), dim3(1), dim3(1024), 0, st, in, n, out, f);
}

// ---- the device-wide form: block sums, the one-launch form over them, the blocks again ----------------------------------------------
// Reduce-then-scan: the input is read twice and the output written once (scan-then-add reads once, writes once, then reads and writes
// all of it again).  A workgroup of 256 threads takes VDJX_SCAN_BLOCK elements, sixteen consecutive ones per thread in the second
// pass, and ONE prefix of the blocks before it (a thread per element that fetched its own block prefix took 197 us for 1.8 M elements).
// The last thread of the last block writes out[n].
template <typename In, typename T, typename F>
__global__ __launch_bounds__(256) void k_scan_sums(const In* __restrict__ in, u32 n, T* __restrict__ sums, F f) {
	__shared__ T part[4];
	const u32 b0 = blockIdx.x * VDJX_SCAN_BLOCK;
	T s = 0;
	for (u32 i = threadIdx.x; i < VDJX_SCAN_BLOCK; i += 256) s += b0 + i < n ? (T) f(in[b0 + i]) : (T) 0;
	s = vdjx_scan_wave(s);
	if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = s;
	__syncthreads();
	if (threadIdx.x == 0) sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
template <typename In, typename T, typename F>
__global__ __launch_bounds__(256) void k_scan_apply(const In* __restrict__ in, u32 n, const T* __restrict__ sum_start, T* __restrict__ out, F f) {
	constexpr u32 PER = VDJX_SCAN_BLOCK / 256u;
	__shared__ T part[4];
	const u32 b0 = blockIdx.x * VDJX_SCAN_BLOCK + threadIdx.x * PER;
	T loc[PER], s = 0;
#pragma unroll
	for (u32 i = 0; i < PER; i++) { loc[i] = s; s += b0 + i < n ? (T) f(in[b0 + i]) : (T) 0; }
	const T incl = vdjx_scan_wave(s);
	if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = incl;
	__syncthreads();
	T base = sum_start[blockIdx.x] + incl - s;
	for (u32 w = 0; w < (threadIdx.x >> 6); w++) base += part[w];
#pragma unroll
	for (u32 i = 0; i < PER; i++) if (b0 + i < n) out[b0 + i] = base + loc[i];
	if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) out[n] = base + s;
}

// the two temporaries (the block sums and their prefix) come out of the caller's workspace: a vdjx_work, or what allocates like one
template <typename A, typename In, typename T, typename F = vdjx_scan_identity>
inline int vdjx_scan_wide(A& db, hipStream_t st, const In* in, u32 n, T* out, F f = F()) {
	if (n == 0) { vdjx_scan_one(st, in, 0u, out, f); return VDJX_OK; }
	const u32 nb = (n + VDJX_SCAN_BLOCK - 1) / VDJX_SCAN_BLOCK;
	T *sums, *sum_start;
	HIP_TRY(db.alloc(&sums, nb));
	HIP_TRY(db.alloc(&sum_start, nb + 1));
	hipLaunchKernelGGL((k_scan_sums<In, T, F>), dim3(nb), dim3(256), 0, st, in, n, sums, f);
	vdjx_scan_one(st, (const T*) sums, nb, sum_start);
	hipLaunchKernelGGL((k_scan_apply<In, T, F>), dim3(nb), dim3(256), 0, st, in, n, (const T*) sum_start, out, f);
	return VDJX_OK;
}

}  // namespace
