// vdjx_diversity.hip -- bootstrap clonal diversity: the Hill curve D(q) of the clone abundances, resampled to a common depth
// (gfx950 only, wave64).
//
//   vdjx_diversity   B replicates of N draws from the cumulative table of the weights, a count matrix B x C, then the Hill numbers of
//               every replicate at Q orders (the model: include/vdjx.h; in Python: tests/diversity_model.py)
//
// The host sums the weights (at most 2^20 of them) into cum[0 .. C] and takes the replicates in batches of max(1, floor(cells / C))
// whole replicates (VDJX_DIV_CELLS).  A batch is a memset of its counts and three dispatches, whatever B, C and N are:
//   k_div_draw   grid (slices, replicates), 1,024 threads.  A workgroup owns a slice of one replicate's draws: draw i is
//                u = mix64(mix64(seed) + (r << 32 | i)), t = the high half of u * W, and the clone is the largest k with cum[k] <= t.
//                The search starts in a coarse table in LDS (every `stride`-th cum, at most 1,024 entries: all of cum when C <= 1,024)
//                and ends in the segment of at most `stride` entries in global memory.  When C <= VDJX_DIV_LDS_CLONES (at most
//                16,384 counters: 64 KiB beside the table's 8 KiB, two workgroups per CU) the workgroup counts in LDS with integer
//                atomics and flushes its non-zero bins with one global atomicAdd each; otherwise every draw is a global atomicAdd.
//                Integer adds only: the counts do not depend on the order they land in.
//   k_div_hill   grid (P, replicates), 256 threads, over a replicate's counts (or, once, over the weights: `observed`).  A workgroup
//                takes every P-th tile of 256 values: a thread loads one, forms p and ln p, and the non-zero ones are compacted into LDS
//                in index order.  Then thread t sums ONE order, j = t % Q, over the tile's entries g, g + G, ... (g = t / Q, G =
//                floor(256 / Q)): one accumulator per thread, no array of sums, and a value is read from global memory once for all Q
//                orders.  At the end the G accumulators of an order are added in the order of g: the workgroup's partial.
//   k_div_fin    a thread per (replicate, order): the P partials in workgroup order, then q = 0: the sum; q = 1: exp(-sum);
//                otherwise sum^(1 / (1 - q)).
// No atomics on doubles: every sum is stored and summed in a fixed order, two calls give the same bits.  Only out_d and, if asked
// for, the counts come back; mean and sd are summed on the host in replicate order.
#include "vdjx_common.h"

#include <algorithm>
#include <math.h>
#include <string.h>

#define DIV_DRAW_THREADS 1024u
#define DIV_COARSE 1024u                 // entries of the coarse table: 8 KiB
#define DIV_LDS_MAX 16384u               // counters of the LDS histogram: 64 KiB; with the table 73,728 bytes, two workgroups in a CU's 160 KiB
#define DIV_HILL_THREADS 256u
#define DIV_HILL_WG 32u                  // at most this many workgroups (partials) per replicate
#define DIV_TARGET_WG 1024u              // draw workgroups aimed at: two rounds of two per CU

// cum[0 .. C) is read (cum[C] = W > t never has to be); seedmix = mix64(seed); replicate r = r0 + blockIdx.y + 1
template <bool LDS_HIST>
__global__ __launch_bounds__(1024) void k_div_draw(const u64* __restrict__ cum, u32 C, u32 stride, u32 ncoarse, u64 W, u64 seedmix, u32 r0, u32 N,
                                                   u32 per_slice, u32* __restrict__ counts) {
	__shared__ u64 coarse[DIV_COARSE];
	__shared__ u32 hist[LDS_HIST ? DIV_LDS_MAX : 1u];
	const u32 tid = threadIdx.x;
	for (u32 j = tid; j < ncoarse; j += DIV_DRAW_THREADS) coarse[j] = cum[(size_t) j * stride];
	if (LDS_HIST)
		for (u32 k = tid; k < C; k += DIV_DRAW_THREADS) hist[k] = 0;
	__syncthreads();
	u32* mine = counts + (size_t) blockIdx.y * C;
	const u64 r = (u64) r0 + blockIdx.y + 1u;
	const u64 begin = (u64) blockIdx.x * per_slice, end = min(begin + per_slice, (u64) N);
	for (u64 i = begin + tid; i < end; i += DIV_DRAW_THREADS) {
		const u64 u = vdjx_mix64(seedmix + (r << 32 | i));
		const u64 t = __umul64hi(u, W);                     // < W
		u32 lo = 0, hi = ncoarse;                          // coarse[0] = 0 <= t: the largest j with coarse[j] <= t
		while (hi - lo > 1u) {
			const u32 mid = (lo + hi) >> 1;
			if (coarse[mid] <= t) lo = mid; else hi = mid;
		}
		lo *= stride;                                      // cum[lo] <= t, and cum[lo + stride] > t where it exists
		hi = min(lo + stride, C);
		while (hi - lo > 1u) {
			const u32 mid = (lo + hi) >> 1;
			if (cum[mid] <= t) lo = mid; else hi = mid;
		}
		if (LDS_HIST) atomicAdd(&hist[lo], 1u);
		else atomicAdd(&mine[lo], 1u);
	}
	if (LDS_HIST) {
		__syncthreads();
		for (u32 k = tid; k < C; k += DIV_DRAW_THREADS) {
			const u32 h = hist[k];
			if (h) atomicAdd(&mine[k], h);
		}
	}
}

// vals: `C` values per replicate (blockIdx.y), p = value / denom; partial[(replicate * P + workgroup) * Q + j]
template <typename T>
__global__ __launch_bounds__(256) void k_div_hill(const T* __restrict__ vals, u32 C, double denom, const double* __restrict__ q, u32 Q, u32 P,
                                                  double* __restrict__ partial) {
	__shared__ double p_tile[DIV_HILL_THREADS], l_tile[DIV_HILL_THREADS], red[DIV_HILL_THREADS];
	__shared__ u32 wave_n[DIV_HILL_THREADS / 64u];
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u32 G = DIV_HILL_THREADS / Q, j = tid % Q, g = tid / Q;
	const bool active = g < G;
	const double qj = q[j];
	const T* mine = vals + (size_t) blockIdx.y * C;
	double acc = 0.0;
	for (u32 base = blockIdx.x * DIV_HILL_THREADS; base < C; base += P * DIV_HILL_THREADS) {      // (the bounds are the workgroup's: every thread takes every turn)
		const u32 idx = base + tid;
		const T c = idx < C ? mine[idx] : (T) 0;
		const bool nz = c != 0;
		const double p = (double) c / denom;
		const u64 b = __ballot(nz);
		if (lane == 0) wave_n[wave] = (u32) __popcll(b);
		__syncthreads();
		u32 at = (u32) __popcll(b & ((1ull << lane) - 1ull)), total = 0;
		for (u32 w = 0; w < DIV_HILL_THREADS / 64u; w++) {
			if (w < wave) at += wave_n[w];
			total += wave_n[w];
		}
		if (nz) {
			p_tile[at] = p;
			l_tile[at] = log(p);
		}
		__syncthreads();
		if (active)
			for (u32 e = g; e < total; e += G) {
				const double pe = p_tile[e];
				acc += qj == 0.0 ? 1.0 : qj == 1.0 ? pe * l_tile[e] : pow(pe, qj);
			}
		__syncthreads();
	}
	red[tid] = active ? acc : 0.0;
	__syncthreads();
	if (tid < Q) {
		double s = 0.0;
		for (u32 k = 0; k < G; k++) s += red[k * Q + tid];
		partial[((size_t) blockIdx.y * P + blockIdx.x) * Q + tid] = s;
	}
}

__global__ __launch_bounds__(256) void k_div_fin(const double* __restrict__ partial, const double* __restrict__ q, u32 Q, u32 P, u32 reps,
                                                 double* __restrict__ d) {
	const u32 t = blockIdx.x * 256u + threadIdx.x;
	if (t >= reps * Q) return;
	const u32 rep = t / Q, j = t % Q;
	double s = 0.0;
	for (u32 w = 0; w < P; w++) s += partial[((size_t) rep * P + w) * Q + j];
	const double qj = q[j];
	d[t] = qj == 0.0 ? s : qj == 1.0 ? exp(-s) : pow(s, 1.0 / (1.0 - qj));
}

static inline u32 div_hill_wgs(u32 C) { return std::min(DIV_HILL_WG, (C + DIV_HILL_THREADS - 1u) / DIV_HILL_THREADS); }

extern "C" int vdjx_diversity(vdjx_ctx* c, const uint64_t* weight, size_t C, const double* q, size_t Q, const vdjx_diversity_params* params,
                              double* out_observed, double* out_d, double* out_mean, double* out_sd, uint32_t* out_counts, vdjx_diversity_info* info) {
	static const char* who = "vdjx_diversity";
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (C == 0) return VDJX_OK;
	if (!weight || !q || !params) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (!out_observed) { vdjx_set_error("%s: NULL argument (out_observed)", who); return VDJX_EINVAL; }
	if (!out_d) { vdjx_set_error("%s: NULL argument (out_d)", who); return VDJX_EINVAL; }
	if (!out_mean || !out_sd) { vdjx_set_error("%s: NULL argument (%s)", who, out_mean ? "out_sd" : "out_mean"); return VDJX_EINVAL; }
	if (C >= (1ull << 20)) { vdjx_set_error("%s: %zu clones (at most 2^20 - 1 per call)", who, C); return VDJX_EINVAL; }
	if (params->replicates < 1 || params->replicates > 4096) { vdjx_set_error("%s: %u replicates (1 .. 4096)", who, params->replicates); return VDJX_EINVAL; }
	if (params->depth < 1 || params->depth > 0x7FFFFFFFu) { vdjx_set_error("%s: a depth of %u draws (1 .. 2^31 - 1)", who, params->depth); return VDJX_EINVAL; }
	if (Q < 1 || Q > 64) { vdjx_set_error("%s: %zu orders (1 .. 64)", who, Q); return VDJX_EINVAL; }
	for (size_t j = 0; j < Q; j++) {
		if (!(q[j] >= 0.0 && q[j] <= 16.0)) { vdjx_set_error("%s: order %zu is %g (0 .. 16)", who, j, q[j]); return VDJX_EINVAL; }
		const double off = fabs(q[j] - 1.0);
		if (off > 0.0 && off < 1.0 / 64.0) { vdjx_set_error("%s: order %zu is %.17g, within 1/64 of 1 but not 1", who, j, q[j]); return VDJX_EINVAL; }
	}
	const auto t0 = std::chrono::steady_clock::now();
	const u32 nC = (u32) C, nQ = (u32) Q, B = params->replicates, N = params->depth;
	vdjx_diversity_info inf;
	memset(&inf, 0, sizeof inf);
	std::vector<u64> cum(C + 1);
	cum[0] = 0;
	for (size_t k = 0; k < C; k++) {
		if (weight[k] > 0x7FFFFFFFFFFFFFFFull - cum[k]) { vdjx_set_error("%s: the weights sum to 2^63 or more (at clone %zu)", who, k); return VDJX_EINVAL; }
		cum[k + 1] = cum[k] + weight[k];
		inf.weighted += weight[k] != 0;
	}
	const u64 W = cum[C];
	if (W == 0) { vdjx_set_error("%s: %zu clones of weight 0", who, C); return VDJX_EINVAL; }
	const u64 cells = (u64) vdjx_env_num("VDJX_DIV_CELLS", 1ll << 28, 1, 1ll << 30);
	const u32 lds_max = (u32) vdjx_env_num("VDJX_DIV_LDS_CLONES", DIV_LDS_MAX, 0, DIV_LDS_MAX);
	const bool lds = nC <= lds_max;
	const u32 per_batch = (u32) std::min<u64>(B, std::max<u64>(1, cells / C));
	const u32 stride = (nC + DIV_COARSE - 1u) / DIV_COARSE, ncoarse = (nC + stride - 1u) / stride;      // stride >= 1, ncoarse <= 1,024
	const u32 P = div_hill_wgs(nC);
	inf.clones = nC;
	inf.weight = W;
	inf.depth = N;
	inf.replicates = B;
	inf.path = lds ? VDJX_DIV_PATH_LDS : VDJX_DIV_PATH_GLOBAL;

	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	vdjx_work wk(c);
	u64 *d_cum, *d_weight;
	u32* d_counts;
	double *d_q, *d_partial, *d_d;
	HIP_TRY(wk.alloc(&d_cum, C + 1));
	HIP_TRY(wk.alloc(&d_weight, C));
	HIP_TRY(wk.alloc(&d_q, Q));
	HIP_TRY(wk.alloc(&d_counts, (size_t) per_batch * C));
	HIP_TRY(wk.alloc(&d_partial, (size_t) per_batch * P * Q));
	HIP_TRY(wk.alloc(&d_d, (size_t) per_batch * Q));
	HIP_TRY(hipMemcpyAsync(d_cum, cum.data(), (C + 1) * sizeof(u64), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_weight, weight, C * sizeof(u64), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_q, q, Q * sizeof(double), hipMemcpyHostToDevice, st));
	// observed: the same two kernels over the weights themselves
	{
		vdjx_prof_scope ps(c, "k_div_hill");
		hipLaunchKernelGGL(k_div_hill<u64>, dim3(P, 1), dim3(DIV_HILL_THREADS), 0, st, (const u64*) d_weight, nC, (double) W, (const double*) d_q, nQ, P, d_partial);
	}
	{
		vdjx_prof_scope ps(c, "k_div_fin");
		hipLaunchKernelGGL(k_div_fin, dim3((nQ + 255u) / 256u), dim3(256), 0, st, (const double*) d_partial, (const double*) d_q, nQ, P, 1u, d_d);
	}
	HIP_TRY(hipMemcpyAsync(out_observed, d_d, Q * sizeof(double), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	const u64 seedmix = vdjx_mix64(params->seed);
	for (u32 r0 = 0; r0 < B; r0 += per_batch) {
		const u32 reps = std::min(per_batch, B - r0);
		// slices of a replicate: enough workgroups to fill the device, but every one with draws to speak of (the LDS path: four per counter it flushes)
		const u64 least = lds ? std::max<u64>(4096, 4ull * nC) : 4096;
		const u32 slices = (u32) std::max<u64>(1, std::min<u64>((DIV_TARGET_WG + reps - 1u) / reps, N / least));
		const u32 per_slice = (u32) (((u64) N + slices - 1u) / slices);
		HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t) reps * C * sizeof(u32), st));
		{
			vdjx_prof_scope ps(c, "k_div_draw");
			if (lds)
				hipLaunchKernelGGL(k_div_draw<true>, dim3(slices, reps), dim3(DIV_DRAW_THREADS), 0, st, (const u64*) d_cum, nC, stride, ncoarse, W, seedmix, r0, N, per_slice, d_counts);
			else
				hipLaunchKernelGGL(k_div_draw<false>, dim3(slices, reps), dim3(DIV_DRAW_THREADS), 0, st, (const u64*) d_cum, nC, stride, ncoarse, W, seedmix, r0, N, per_slice, d_counts);
		}
		{
			vdjx_prof_scope ps(c, "k_div_hill");
			hipLaunchKernelGGL(k_div_hill<u32>, dim3(P, reps), dim3(DIV_HILL_THREADS), 0, st, (const u32*) d_counts, nC, (double) N, (const double*) d_q, nQ, P, d_partial);
		}
		{
			vdjx_prof_scope ps(c, "k_div_fin");
			hipLaunchKernelGGL(k_div_fin, dim3((reps * nQ + 255u) / 256u), dim3(256), 0, st, (const double*) d_partial, (const double*) d_q, nQ, P, reps, d_d);
		}
		HIP_TRY(hipMemcpyAsync(out_d + (size_t) r0 * Q, d_d, (size_t) reps * Q * sizeof(double), hipMemcpyDeviceToHost, st));
		if (out_counts) HIP_TRY(hipMemcpyAsync(out_counts + (size_t) r0 * C, d_counts, (size_t) reps * C * sizeof(u32), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(hipGetLastError());
		vdjx_prof_collect(c, false);
		inf.batches++;
	}
	// mean and sd (n - 1) over the replicates, in replicate order
	for (size_t j = 0; j < Q; j++) {
		double s = 0.0, v = 0.0;
		for (u32 r = 0; r < B; r++) s += out_d[(size_t) r * Q + j];
		const double mean = s / (double) B;
		for (u32 r = 0; r < B; r++) {
			const double e = out_d[(size_t) r * Q + j] - mean;
			v += e * e;
		}
		out_mean[j] = mean;
		out_sd[j] = B > 1 ? sqrt(v / (double) (B - 1)) : 0.0;
	}
	if (info) *info = inf;
	c->stats["diversity_batches"] = inf.batches;
	c->stats["diversity_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}
