// vdjx_selpost.h -- the posterior of sigma on the 4,001-point grid, shared by vdjx_select.hip (vdjx_selection: one binomial likelihood per
// row) and vdjx_selconv.hip (vdjx_selection_convolve: the members' own posteriors, convolved).  What is here is what both calls must agree
// on: how a count row becomes a member (sel_member), the order of the members of a group (sel_group_order), a member's terms at a grid
// point (sel_terms), and the finish of a row from its unnormalised grid values (sel_finish_tail: the sum, the CDF and its two quantile
// indices, sigma, p_positive, the 72-byte stat and the density).  The model: include/vdjx.h.
#pragma once
#include "vdjx_common.h"

#include <math.h>

#define SEL_T VDJX_SEL_GRID
#define SEL_PER 16                       // grid points a thread of a 256-thread finish owns: 256 * 16 >= 4001

struct SelMember { u32 x, n; double lo; };            // a contig in a region: x of n, ln exp_r - ln sum exp_s; n = 0: adds nothing
static_assert(sizeof(SelMember) == 16 && sizeof(vdjx_sel_counts) == 64 && sizeof(vdjx_sel_stat) == 72, "uploaded / returned as they are");

// ---- the host's side -----------------------------------------------------------------------------------------------------------------------
// contig r's member in region k of K: it contributes where n > 0, exp_r[k] > 0 and the sum of exp_s > 0; *es: that sum
static inline SelMember sel_member(const vdjx_sel_counts& r, u32 k, u32 K, u64* es_out = nullptr) {
	u64 ss = 0, es = 0;
	for (u32 j = 0; j < K; j++) { ss += (u64) r.obs_s[j]; es += r.exp_s[j]; }
	const u64 x = (u64) r.obs_r[k], nn = x + ss;
	SelMember e = {0u, 0u, 0.0};
	if (nn > 0 && r.exp_r[k] > 0 && es > 0) { e.x = (u32) x; e.n = (u32) nn; e.lo = log((double) r.exp_r[k]) - log((double) es); }
	if (es_out) *es_out = es;
	return e;
}

// the grouped contigs by group, contig order inside a group (a counting sort): gstart[G + 1], gorder[the grouped contigs]
static inline void sel_group_order(const int32_t* group, size_t n, u32 G, std::vector<u32>& gstart, std::vector<u32>& gorder) {
	gstart.assign(G + 1, 0);
	gorder.clear();
	if (!G) return;
	for (size_t i = 0; i < n; i++)
		if (group[i] >= 0) gstart[(u32) group[i] + 1]++;
	for (u32 g = 0; g < G; g++) gstart[g + 1] += gstart[g];
	gorder.resize(gstart[G]);
	std::vector<u32> at(gstart.begin(), gstart.end() - 1);
	for (size_t i = 0; i < n; i++)
		if (group[i] >= 0) gorder[at[(u32) group[i]]++] = (u32) i;
}

// ---- the device's side ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sel_softplus(double z) { return fmax(z, 0.0) + log1p(exp(-fabs(z))); }
__device__ __forceinline__ double sel_sigma(int t) { return (double) (t - 2000) / 100.0; }

// the members' terms at one grid point, in member order, from 0
__device__ __forceinline__ double sel_terms(const SelMember* __restrict__ m, u32 count, double sg) {
	double acc = 0.0;
	for (u32 k = 0; k < count; k++) {
		const SelMember e = m[k];            // (uniform across the workgroup)
		if (e.n == 0) continue;
		const double z = sg + e.lo;
		acc += (double) e.x * z - (double) e.n * sel_softplus(z);
	}
	return acc;
}

__device__ __forceinline__ double sel_shfl_xor(double v, int o) {
	return __longlong_as_double((long long) vdjx_shfl_xor64((u64) __double_as_longlong(v), o));
}

// the block's sum / maximum of one value per thread, in a fixed order: inside a wave by a butterfly, the four waves in order
__device__ __forceinline__ double sel_block_sum(double v, double* red) {
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) v += sel_shfl_xor(v, o);
	__syncthreads();
	if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double sel_block_max(double v, double* red) {
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) v = fmax(v, sel_shfl_xor(v, o));
	__syncthreads();
	if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// The finish of a row by a 256-thread workgroup: thread tid holds the unnormalised values f of the grid points 16 tid .. 16 tid + 15 (0
// past the grid).  ell[SEL_T], tot[256], red[4] and qidx[2][4] are the workgroup's LDS; sequences .. exp_s are the row's counts (scalars:
// a 72-byte stat passed by value went through scratch).  Writes *out_stat and, where pdf is not NULL, the density f / (0.01 S) to
// pdf[SEL_T].  Every thread of the workgroup calls it.
__device__ __forceinline__ void sel_finish_tail(const double (&f)[SEL_PER], double* ell, double* tot, double* red, int (*qidx)[4], u32 sequences,
                                                u64 sx, u64 sn, u64 exp_r, u64 exp_s, vdjx_sel_stat* __restrict__ out_stat,
                                                double* __restrict__ pdf) {
	const u32 tid = threadIdx.x;
	const int t0 = (int) tid * SEL_PER;
	double loc = 0.0, sw = 0.0, pos = 0.0;
#pragma unroll
	for (int j = 0; j < SEL_PER; j++) {
		const int t = t0 + j;
		loc += f[j];
		sw += sel_sigma(t) * f[j];
		pos += t > 2000 ? f[j] : t == 2000 ? 0.5 * f[j] : 0.0;
	}
	// the exclusive scan of the threads' totals: the wave's by shuffles, the waves' in order
	double inc = loc;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const long long b = __double_as_longlong(inc);
		const u32 lo = (u32) __shfl_up((int) (u32) b, o, 64), hi = (u32) __shfl_up((int) (u32) ((u64) b >> 32), o, 64);
		const double up = __longlong_as_double((long long) ((u64) hi << 32 | lo));
		if ((int) (tid & 63u) >= o) inc += up;
	}
	tot[tid] = inc;
	__syncthreads();
	const u32 wv = tid >> 6;
	double base = 0.0;
	for (u32 k = 0; k < wv; k++) base += tot[64 * k + 63];
	const double S = ((tot[63] + tot[127]) + tot[191]) + tot[255];
	double run = base + (inc - loc);
	int first[2] = {SEL_T, SEL_T};
#pragma unroll
	for (int j = 0; j < SEL_PER; j++) {
		run += f[j];
		const double cdf = run / S;
		const int t = t0 + j;
		if (t < SEL_T) {
			if (cdf >= 0.025 && first[0] == SEL_T) first[0] = t;
			if (cdf >= 0.975 && first[1] == SEL_T) first[1] = t;
		}
	}
#pragma unroll
	for (int k = 0; k < 2; k++) {
		int v = first[k];
#pragma unroll
		for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
		if ((tid & 63u) == 0) qidx[k][wv] = v;
	}
	const double ssum = sel_block_sum(sw, red);      // (its barriers publish qidx)
	const double psum = sel_block_sum(pos, red);
	if (tid == 0) {
		int qi[2];
		for (int k = 0; k < 2; k++) qi[k] = min(min(min(qidx[k][0], qidx[k][1]), min(qidx[k][2], qidx[k][3])), SEL_T - 1);
		vdjx_sel_stat s;
		s.sequences = sequences;
		s.pad = 0;
		s.x = sx; s.n = sn; s.exp_r = exp_r; s.exp_s = exp_s;
		s.sigma = ssum / S;
		s.lower = sel_sigma(qi[0]);
		s.upper = sel_sigma(qi[1]);
		s.p_positive = psum / S;
		*out_stat = s;
	}
	if (pdf) {
		const double den = 0.01 * S;
		__syncthreads();                     // (pdf is the workgroup's: all of it comes here)
#pragma unroll
		for (int j = 0; j < SEL_PER; j++)
			if (t0 + j < SEL_T) ell[t0 + j] = f[j] / den;
		__syncthreads();
		for (int t = (int) tid; t < SEL_T; t += 256) pdf[t] = ell[t];      // (through LDS: neighbouring threads store neighbouring doubles)
	}
}
