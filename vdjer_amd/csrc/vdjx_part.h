// vdjx_part.h -- the LDS-staged partition of the k-mer build (software write combining): elements -> runs of their buckets.
//
// A direct scatter into 2^15 buckets writes 4-16 B at a time to tens of millions of open write fronts; rocprofv3 WRITE_SIZE showed
// 5.7x the algorithmic bytes reaching HBM (profiles/r01b_traffic.json).  Instead a workgroup of PART_THREADS takes a ROUND of elements
// (what fits the PART_LDS_BYTES stage), counts them per bucket in LDS, reserves one run per bucket from the pass's global cursors,
// places them bucket by bucket in the stage and writes every run with consecutive lanes on consecutive addresses.  <= PART_MAXB buckets
// per pass keep the runs long; more are reached in two passes, the second working inside one segment of the first (a few MB, cache
// resident) at a time.  Placement inside a bucket is arbitrary (the cursor bumps of the rounds race): what reads the buckets is order-free.
//
//   part_round   the bookkeeping of a round: begin, (count,) reserve, (slot,) flush.  k_part_records_g (vdjx_kmer.hip) counts, places
//                and -- where it keeps its tuples with their buckets -- copies out itself; the rest of its round is this.  Where the buckets are capacities and not
//                exact sizes (the k-mer build's sampled cut), limits names where they end and reserve refuses a run past its end
//   part_slice   the share of a workgroup in a pass over segments; k_seg_hist_g counts the sub-buckets of the same slices
//   k_part       the streaming pass: T elements in, T elements out, the bucket from a functor on the element, the range from
//                part_share (one level, or the first of two) or part_segs (the second level)
//   part_launch  the cursors from the bucket starts, the dynamic LDS attribute and the launch of one pass
// Everything here has internal linkage.  The test suite reaches k_part and part_launch through vdjx_part_u64 (include/vdjx.h; defined in
// vdjx_kmer.hip, the file that includes this).
#pragma once

#include "vdjx_common.h"

#include <type_traits>

#define PART_THREADS 1024
#define PART_LDS_BYTES 131072
#define PART_MAXB 1024
#define PART_SLICES 8u              // workgroups per coarse bucket in the second pass of the tuples (k_seg_hist_g, k_part over part_segs)
#define PART_NONE 0xFFFFFFFFu       // the bucket of an element that is not there
#define PART_HOLE 0xFFFFFFFFFFFFFFFFull      // the 8-byte element that the paired-load form of k_part drops
#define PART_DEAD 0xFFFFFFFFu       // what reserve returns once a bucket of the pass has run over its limit: the workgroup stops

namespace {

// exclusive scan of cnt[0..n) (n <= 1024) into base[0..n], base[n] = total; all PART_THREADS threads call it.
// Two counts per thread, DPP prefix sums inside the waves, one wave for the wave totals: three barriers instead of twenty.
__device__ inline void part_scan(const u32* cnt, u32* base, u32* tmp, u32 n) {
	const u32 t = threadIdx.x, lane = t & 63, wv = t >> 6;
	const u32 a = 2 * t < n ? cnt[2 * t] : 0, b = 2 * t + 1 < n ? cnt[2 * t + 1] : 0;
	const u32 incl = (u32) vdjx_wave_scan_add((int) (a + b));
	if (lane == 63) tmp[wv] = incl;
	__syncthreads();
	if (wv == 0) {
		const u32 w = lane < PART_THREADS / 64 ? tmp[lane] : 0;
		const u32 wi = (u32) vdjx_wave_scan_add((int) w);
		if (lane < PART_THREADS / 64) tmp[lane] = wi - w;          // exclusive offset of every wave
		if (lane == 63) tmp[PART_THREADS / 64] = wi;               // grand total
	}
	__syncthreads();
	const u32 excl = tmp[wv] + incl - (a + b);
	if (2 * t < n) base[2 * t] = excl;
	if (2 * t + 1 < n) base[2 * t + 1] = excl + a;
	if (t == 0) base[n] = tmp[PART_THREADS / 64];
	__syncthreads();
}

// an element's own load and store: Tup16 / Tup24 bring theirs, an item is a word
template <typename T> __device__ inline T part_load(const T* p) { return T::load(p); }
template <typename T> __device__ inline void part_store(T* p, const T& x) { T::store(p, x); }
__device__ inline u64 part_load(const u64* p) { return *p; }
__device__ inline void part_store(u64* p, const u64& x) { *p = x; }

// One round of a workgroup, declared once per kernel as a __shared__ object.  begin, reserve and flush are called by all PART_THREADS
// threads; between them the kernel counts every element of the round once (count) and, after reserve, takes a slot of the stage for
// every one (slot) and stores it there.
struct part_round {
	u32 cnt[PART_MAXB], base[PART_MAXB + 1], cur[PART_MAXB], gbase[PART_MAXB];
	u32 tmp[PART_THREADS / 64 + 1];                 // (part_scan: the waves' totals and the grand total)
	u32 end[PART_MAXB];           // (limits) where the workgroup's buckets end
	u32* over;
	u32 dead, stop;

	// Once per workgroup, before its first round, by all threads -- only in a pass whose buckets are laid out by CAPACITIES (the sampled
	// cut of the k-mer build): bucket i ends before lim[(i + 1) << lsh].  A round with a run that would cross its limit sets the word
	// `word`, and reserve returns PART_DEAD: the workgroup must write nothing of it (the rounds that fit write where they may; what reads
	// the pass's output looks at the word first).  The rounds do NOT poll the word: a workgroup goes on until a run of its own would
	// cross a limit -- every writer checks its own runs, so nothing is written past a limit either way.  The limits stay in LDS: a
	// workgroup's buckets are the same in all its rounds.  lim == nullptr: the buckets are exact, nothing is checked.
	// `seen`: a word that says the pass's INPUT is void (an earlier pass ran over; it may be the word this pass sets itself, and then
	// changes while the kernel runs).  ONE thread reads it, and the answer -- true: the workgroup returns at once, all of it -- is the
	// same in every thread: waves of one workgroup that read the word for themselves could disagree, and those that went on would
	// scan and flush counts the others never cleared.
	__device__ inline bool limits(u32 nbk, const u32* __restrict__ lim, u32 lsh, u32* word, const u32* seen = nullptr) {
		if (lim) for (u32 i = threadIdx.x; i < nbk; i += PART_THREADS) end[i] = lim[((size_t) i + 1) << lsh];
		if (threadIdx.x == 0) {
			over = lim ? word : nullptr;
			stop = seen ? __hip_atomic_load(seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
		}
		__syncthreads();
		return stop != 0;
	}

	__device__ inline void begin(u32 nbk) {
		for (u32 i = threadIdx.x; i < nbk; i += PART_THREADS) cnt[i] = 0;
		if (threadIdx.x == 0) dead = 0;
		__syncthreads();
	}
	__device__ inline void count(u32 b) { atomicAdd(&cnt[b], 1u); }
	// after a barrier behind the last count: the buckets' places in the stage and their runs in the output, bucket i's from gcur[i];
	// returns the number of elements of the round, or PART_DEAD (limits)
	__device__ inline u32 reserve(u32 nbk, u32* __restrict__ gcur) {
		part_scan(cnt, base, tmp, nbk);
		u32* const word = over;
		for (u32 i = threadIdx.x; i < nbk; i += PART_THREADS) {
			cur[i] = base[i];
			const u32 n = cnt[i];
			const u32 g = n ? atomicAdd(&gcur[i], n) : 0u;
			gbase[i] = g;
			if (word && (u64) g + n > (u64) end[i]) { dead = 1; atomicExch(word, 1u); }
		}
		__syncthreads();
		return dead ? PART_DEAD : base[nbk];
	}
	__device__ inline u32 slot(u32 b) { return atomicAdd(&cur[b], 1u); }
	// after a barrier behind the last store to the stage: the n staged elements to their runs (the bucket again from the element)
	template <typename T, typename Key> __device__ inline void flush(const T* stage, u32 n, T* __restrict__ out, const Key& key) {
		for (u32 i = threadIdx.x; i < n; i += PART_THREADS) {
			const T x = part_load(&stage[i]);
			const u32 b = key(x);
			part_store(&out[gbase[b] + (i - base[b])], x);
		}
		__syncthreads();
	}
};

// a pass over segments with `slices` workgroups each: workgroup blockIdx.x has slice blockIdx.x % slices of segment blockIdx.x / slices,
// which is [seg_start[seg << seg_shift], seg_start[(seg + 1) << seg_shift]) -- or, where the earlier pass filled a layout of capacities,
// ends at seg_end[seg], the cursor that pass left.  Returns the segment; [t0, t1) is empty for a slice that gets nothing.
__device__ inline u32 part_slice(const u32* __restrict__ seg_start, u32 seg_shift, u32 slices, size_t& t0, size_t& t1, const u32* __restrict__ seg_end = nullptr) {
	const u32 seg = blockIdx.x / slices, sl = blockIdx.x % slices;
	const size_t s0 = seg_start[(size_t) seg << seg_shift], s1 = seg_end ? seg_end[seg] : seg_start[((size_t) seg + 1) << seg_shift];
	const size_t per = (s1 - s0 + slices - 1) / slices;
	t0 = s0 + (size_t) sl * per;
	t1 = t0 + per < s1 ? t0 + per : s1;
	return seg;
}

// The ranges of k_part: [t0, t1) of the input for this workgroup, its number of buckets and (returned) its first cursor.
// part_share: an even share of [0, *n) in whole rounds (so every share starts on an even element), nbk buckets, any number <= PART_MAXB.
struct part_share {
	const unsigned long long* n;          // read on the device: the pass need not wait for the host to know it
	u32 nbk;
	__device__ inline size_t span(u32 round, size_t& t0, size_t& t1, u32& buckets) const {
		const size_t N = (size_t) *n;
		const size_t per = ((N + gridDim.x - 1) / gridDim.x + round - 1) / round * round;
		t0 = (size_t) blockIdx.x * per;
		t1 = t0 + per < N ? t0 + per : N;
		buckets = nbk;
		return 0;
	}
	__device__ inline const u32* limits(size_t) const { return nullptr; }
	__device__ inline u32* over_word() const { return nullptr; }
};
// part_segs: a slice of a segment of an earlier pass, cut into 2^sub_bits buckets with cursors of the segment's own.  seg_end: the
// segments' ends where they are not the next segments' starts (part_slice); lim / over: this pass's own buckets have limits, bucket j
// of all of them ends before lim[j + 1] (part_round::reserve)
struct part_segs {
	const u32* seg_start;
	u32 seg_shift, slices, sub_bits;
	const u32* seg_end = nullptr;
	const u32* lim = nullptr;
	u32* over = nullptr;
	__device__ inline size_t span(u32, size_t& t0, size_t& t1, u32& buckets) const {
		buckets = 1u << sub_bits;
		return (size_t) part_slice(seg_start, seg_shift, slices, t0, t1, seg_end) << sub_bits;
	}
	__device__ inline const u32* limits(size_t first) const { return lim ? lim + first : nullptr; }
	__device__ inline u32* over_word() const { return over; }
};

// The streaming pass.  key(element) is its bucket among the workgroup's (below the range's number of buckets).  PAIRED: 8-byte elements
// read two per 16-byte load (the range starts on an even element: part_share) of which the PART_HOLEs are dropped; otherwise one
// part_load per element and every element is kept.
template <typename T, typename Key, typename Range, bool PAIRED = false>
__global__ __launch_bounds__(PART_THREADS) void k_part(const T* __restrict__ in, Range range, Key key, u32* __restrict__ gcur, T* __restrict__ out) {
	extern __shared__ __attribute__((aligned(16))) uint8_t part_smem[];
	T* stage = (T*) part_smem;
	__shared__ part_round pr;
	constexpr u32 PER = PART_LDS_BYTES / sizeof(T) / PART_THREADS;          // elements per thread per round
	constexpr u32 ROUND = PER * PART_THREADS;
	static_assert(!PAIRED || (std::is_same<T, u64>::value && PER % 2 == 0), "the paired loads are for 8-byte elements");
	size_t t0, t1;
	u32 nbk;
	// (the range's word set: the pass before ran over and its cursors bound nothing that may be read, or a workgroup of this pass did and
	// the rest is for nothing.  span reads starts and cursors only; nothing of the input is touched before the workgroup has decided)
	const size_t first = range.span(ROUND, t0, t1, nbk);
	u32* gc = gcur + first;
	if (pr.limits(nbk, range.limits(first), 0u, range.over_word(), range.over_word())) return;      // (uniform)
	for (size_t ts = t0; ts < t1; ts += ROUND) {
		const size_t te = ts + ROUND < t1 ? ts + ROUND : t1;
		pr.begin(nbk);
		T r_x[PER];
		u32 r_b[PER];
		if constexpr (PAIRED) {
#pragma unroll
			for (u32 j = 0; j < PER; j += 2) {                            // 16-byte loads
				const size_t t = ts + ((size_t) (j / 2) * PART_THREADS + threadIdx.x) * 2;
				r_x[j] = PART_HOLE; r_x[j + 1] = PART_HOLE;
				if (t + 1 < te) { const ulonglong2 v = *(const ulonglong2*) &in[t]; r_x[j] = v.x; r_x[j + 1] = v.y; }
				else if (t < te) r_x[j] = in[t];
			}
#pragma unroll
			for (u32 j = 0; j < PER; j++) {
				r_b[j] = PART_NONE;
				if (r_x[j] != PART_HOLE) { r_b[j] = key(r_x[j]); pr.count(r_b[j]); }
			}
		} else {
#pragma unroll
			for (u32 j = 0; j < PER; j++) {
				const size_t t = ts + (size_t) j * PART_THREADS + threadIdx.x;
				r_b[j] = PART_NONE;
				if (t < te) { r_x[j] = part_load(&in[t]); r_b[j] = key(r_x[j]); }
			}
#pragma unroll
			for (u32 j = 0; j < PER; j++) if (r_b[j] != PART_NONE) pr.count(r_b[j]);
		}
		__syncthreads();
		const u32 n = pr.reserve(nbk, gc);
		if (n == PART_DEAD) return;                                   // (uniform)
#pragma unroll
		for (u32 j = 0; j < PER; j++) if (r_b[j] != PART_NONE) part_store(&stage[pr.slot(r_b[j])], r_x[j]);
		__syncthreads();
		pr.flush(stage, n, out, key);
	}
}

// cursors of a partition pass: cur[i] = bucket_start[i << sh]
__global__ void k_init_cursors(const u32* __restrict__ bucket_start, u32 n, u32 sh, u32* __restrict__ cur) {
	u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) cur[i] = bucket_start[(size_t) i << sh];
}

// one pass: its `ncur` cursors gcur[i] = bucket_start[i << sh], then kernel(args..., gcur, out) -- k_part, k_part_records_g -- on `grid`
// workgroups with `lds` bytes of dynamic LDS
template <typename... P, typename O, typename... Args>
inline hipError_t part_launch(hipStream_t st, void (*kernel)(P...), u32 grid, u32 lds, const u32* bucket_start, u32 ncur, u32 sh, u32* gcur, O* out,
                              Args... args) {
	const hipError_t e = hipFuncSetAttribute((const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_init_cursors, dim3((ncur + 255) / 256), dim3(256), 0, st, bucket_start, ncur, sh, gcur);
	hipLaunchKernelGGL(kernel, dim3(grid), dim3(PART_THREADS), lds, st, args..., gcur, out);
	return hipSuccess;
}

}  // namespace
