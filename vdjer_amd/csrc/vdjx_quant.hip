// vdjx_quant.hip -- contig abundances on the device (vdjx_quant, include/vdjx.h): RSEM's core paired-end EM over the placements
// vdjx_map_emit finds for the final contigs, float64 throughout, bitwise reproducible.
//
//   placements   vdjx_map_emit's pairs, kept on the device (contig-major: contig after contig, the reference's order inside a contig)
//   pair-major   counting sort by pair id: degrees (integer atomics), one exclusive scan of (placed << 32 | degree) gives every pair its
//                CSR start and every placed pair its slot; a pair's alignments are then put in ascending contig-major order (rank by
//                counting), so that nothing depends on the order the scatter's atomics ran in.  perm[j] = contig-major index of slot j.
//   weights      the histogram of the inserts of the pairs placed once (integer atomics), P(f) and g(f) in one thread, then per slot
//                its contig and g(f)
//   iteration    E (k_q_estep): one lane per pair of up to Q_LIGHT alignments, the whole wave for a larger pair (a fixed butterfly);
//                r is written to its contig-major place.  M (k_q_mpart, k_q_mfin): every contig's alignments in chunks of Q_CHUNK, a
//                fixed tree per chunk, the chunks of a contig summed in order by one thread, which also takes the stop rule's maximum.
//   stop         k_q_mfin counts the iteration and sets the flag; every kernel of the iteration returns at entry once it is set.  The
//                host enqueues Q_BATCH iterations and looks at the flag once per batch: no grid-wide barrier, no persistent kernel.
#include "vdjx_common.h"
#include "vdjx_scan.h"

#include <algorithm>
#include <math.h>
#include <string.h>

#define Q_MIN_INSERT 50                  // quick_map3.c:23-24, the mapper's window (vdjx_score.hip map_eval_entry)
#define Q_MAX_INSERT 400
#define Q_NBINS (Q_MAX_INSERT - Q_MIN_INSERT + 1)
#define Q_LIGHT 32                       // a pair with more alignments is reduced by the whole wave
#define Q_CHUNK 2048u                    // alignments per workgroup of the M step
#define Q_BATCH 32                       // iterations enqueued between two looks at the flag

struct QState {
	u32 done, iters;
	u64 unique;
	double delta, eff_len;
};

__global__ void k_q_degree(const vdjx_pair* __restrict__ pairs, u32 A, u32 P, u32* __restrict__ deg) {
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A) return;
	const u32 p = pairs[i].pair_id;
	if (p < P) atomicAdd(&deg[p], 1u);
}

// what the scan over the pairs sums (vdjx_scan_wide's load functor): (degree > 0) << 32 | degree.  The exclusive prefix holds the CSR
// start of a pair in the low word, its slot among the placed pairs in the high word; excl[P] = the totals
struct q_deg_key {
	__device__ u64 operator()(u32 d) const { return d ? (1ull << 32) | d : 0ull; }
};

// seg[q] = first slot of placed pair q, seg[placed] = A
__global__ void k_q_csr(const u32* __restrict__ deg, const u64* __restrict__ excl, u32 P, u32* __restrict__ seg) {
	const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p == 0) seg[(u32) (excl[P] >> 32)] = (u32) excl[P];
	if (p < P && deg[p]) seg[(u32) (excl[p] >> 32)] = (u32) excl[p];
}

// every alignment into its pair's range (the degrees count down as cursors): the order inside a range is the atomics', k_q_order fixes it
__global__ void k_q_scatter(const vdjx_pair* __restrict__ pairs, u32 A, u32 P, const u64* __restrict__ excl, u32* __restrict__ cur, u32* __restrict__ tmp) {
	const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A) return;
	const u32 p = pairs[i].pair_id;
	if (p >= P) return;
	tmp[(u32) excl[p] + atomicSub(&cur[p], 1u) - 1u] = i;
}

__device__ inline bool q_in_window(int f) { return f >= Q_MIN_INSERT && f <= Q_MAX_INSERT; }

// a pair's alignments in ascending contig-major index (the rank of each among its pair's: they are distinct), and the inserts of the
// pairs placed once into the histogram
__global__ __launch_bounds__(256) void k_q_order(const u32* __restrict__ seg, u32 Pp, const u32* __restrict__ tmp, const vdjx_pair* __restrict__ pairs,
                                                 u32* __restrict__ perm, u32* __restrict__ hist) {
	__shared__ u32 h[Q_NBINS];
	for (u32 i = threadIdx.x; i < Q_NBINS; i += blockDim.x) h[i] = 0;
	__syncthreads();
	const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
	u32 s = 0, e = 0;
	if (q < Pp) { s = seg[q]; e = seg[q + 1]; }
	const u32 d = e - s;
	if (d == 1) {
		const u32 a = tmp[s];
		perm[s] = a;
		const int f = pairs[a].insert;
		if (q_in_window(f)) atomicAdd(&h[f - Q_MIN_INSERT], 1u);
	} else if (d > 1 && d <= Q_LIGHT) {
		for (u32 j = s; j < e; j++) {
			const u32 x = tmp[j];
			u32 r = 0;
			for (u32 k = s; k < e; k++) r += tmp[k] < x ? 1u : 0u;
			perm[s + r] = x;
		}
	}
	u64 heavy = __ballot(d > Q_LIGHT);
	const u32 lane = threadIdx.x & 63u;
	while (heavy) {
		const int l0 = __ffsll((long long) heavy) - 1;
		heavy &= heavy - 1ull;
		const u32 hs = (u32) __builtin_amdgcn_readlane((int) s, l0), he = (u32) __builtin_amdgcn_readlane((int) e, l0);
		for (u32 j = hs + lane; j < he; j += 64) {
			const u32 x = tmp[j];
			u32 r = 0;
			for (u32 k = hs; k < he; k++) r += tmp[k] < x ? 1u : 0u;
			perm[hs + r] = x;
		}
	}
	__syncthreads();
	for (u32 i = threadIdx.x; i < Q_NBINS; i += blockDim.x)
		if (h[i]) atomicAdd(&hist[i], h[i]);
}

// P(f), g(f) and the effective length, by one thread in a fixed order
__global__ void k_q_gtab(const u32* __restrict__ hist, int L, double* __restrict__ gtab, QState* __restrict__ st) {
	if (threadIdx.x || blockIdx.x) return;
	u64 tot = 0, uniq = 0;
	for (int b = 0; b < Q_NBINS; b++) { tot += (u64) hist[b] + 1ull; uniq += hist[b]; }
	double eff = 0.0;
	for (int b = 0; b < Q_NBINS; b++) {
		const int f = Q_MIN_INSERT + b;
		const double pf = (double) ((u64) hist[b] + 1ull) / (double) tot;
		gtab[b] = f <= L ? pf / (double) (L - f + 1) : 0.0;
		if (f <= L) eff += pf * (double) (L - f + 1);
	}
	st->unique = uniq;
	st->eff_len = eff;
}

// per slot: the contig (off[c] <= a < off[c+1]) and g of the alignment
__global__ void k_q_align(const u32* __restrict__ perm, u32 A, const vdjx_pair* __restrict__ pairs, const u64* __restrict__ off, u32 n,
                          const double* __restrict__ gtab, u32* __restrict__ ct, double* __restrict__ g) {
	const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= A) return;
	const u32 a = perm[j];
	u32 lo = 0, hi = n;
	while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (off[mid] <= a) lo = mid; else hi = mid; }
	ct[j] = lo;
	const int f = pairs[a].insert;
	g[j] = q_in_window(f) ? gtab[f - Q_MIN_INSERT] : 0.0;
}

__global__ void k_q_init(const u64* __restrict__ off, u32 n, double v, double* __restrict__ N) {
	const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c < n) N[c] = off[c + 1] > off[c] ? v : 0.0;
}

// E step: r_a = N_c(a) g_a / (sum over the pair), written to the alignment's contig-major place
__global__ __launch_bounds__(256) void k_q_estep(const QState* __restrict__ st, const u32* __restrict__ seg, u32 Pp, const u32* __restrict__ ct,
                                                 const double* __restrict__ g, const u32* __restrict__ perm, const double* __restrict__ N,
                                                 double* __restrict__ r) {
	if (st->done) return;
	const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
	u32 s = 0, e = 0;
	if (q < Pp) { s = seg[q]; e = seg[q + 1]; }
	const u32 d = e - s;
	if (d >= 1 && d <= Q_LIGHT) {
		double sum = 0.0;
		for (u32 j = s; j < e; j++) sum += N[ct[j]] * g[j];
		for (u32 j = s; j < e; j++) { const double w = N[ct[j]] * g[j]; r[perm[j]] = sum > 0.0 ? w / sum : 0.0; }
	}
	u64 heavy = __ballot(d > Q_LIGHT);
	const u32 lane = threadIdx.x & 63u;
	while (heavy) {
		const int l0 = __ffsll((long long) heavy) - 1;
		heavy &= heavy - 1ull;
		const u32 hs = (u32) __builtin_amdgcn_readlane((int) s, l0), he = (u32) __builtin_amdgcn_readlane((int) e, l0);
		double part = 0.0;
		for (u32 j = hs + lane; j < he; j += 64) part += N[ct[j]] * g[j];
		// a fixed butterfly: every lane ends with the same bits (x + y == y + x)
#pragma unroll
		for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
		for (u32 j = hs + lane; j < he; j += 64) { const double w = N[ct[j]] * g[j]; r[perm[j]] = part > 0.0 ? w / part : 0.0; }
	}
}

// M step, part 1: the sum of r over one chunk of a contig's alignments (a fixed tree)
__global__ __launch_bounds__(256) void k_q_mpart(const QState* __restrict__ st, const uint2* __restrict__ chunks, const double* __restrict__ r,
                                                 double* __restrict__ part) {
	if (st->done) return;
	__shared__ double s[256];
	const uint2 ch = chunks[blockIdx.x];
	double v = 0.0;
	for (u32 i = ch.x + threadIdx.x; i < ch.y; i += 256) v += r[i];
	s[threadIdx.x] = v;
	__syncthreads();
	for (u32 d = 128; d > 0; d >>= 1) {
		if (threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
		__syncthreads();
	}
	if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

// M step, part 2 (one workgroup): N_c = its chunks in order; the stop rule; the iteration is counted
__global__ __launch_bounds__(1024) void k_q_mfin(QState* __restrict__ st, u32 n, const u32* __restrict__ cstart, const double* __restrict__ part,
                                                 const double* __restrict__ Nold, double* __restrict__ Nnew, double tol, u32 max_iter) {
	__shared__ double s[1024];
	const u32 done = st->done;
	if (done) return;
	double mx = 0.0;
	for (u32 c = threadIdx.x; c < n; c += 1024) {
		double v = 0.0;
		for (u32 k = cstart[c]; k < cstart[c + 1]; k++) v += part[k];
		Nnew[c] = v;
		mx = fmax(mx, fabs(v - Nold[c]) / fmax(v, 1.0));
	}
	s[threadIdx.x] = mx;
	__syncthreads();
	for (u32 d = 512; d > 0; d >>= 1) {
		if (threadIdx.x < d) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + d]);
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		const u32 it = st->iters + 1u;
		st->iters = it;
		st->delta = s[0];
		if (s[0] < tol || it >= max_iter) st->done = 1u;
	}
}

static double q_eff_len_uniform(int L) {         // eff_len of a histogram without counts (no placement)
	double eff = 0.0;
	for (int f = Q_MIN_INSERT; f <= Q_MAX_INSERT; f++)
		if (f <= L) eff += (1.0 / (double) Q_NBINS) * (double) (L - f + 1);
	return eff;
}

static double q_us_since(std::chrono::steady_clock::time_point t) {
	return (double) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t).count();
}

// the model over placements that are on the device already (contig-major, offs[n + 1] on the host): what both entries run.  t_map: when
// the caller began to map (nullptr: it did not, quant_map_us is 0)
static int q_run(vdjx_ctx* c, vdjx_work& db, const vdjx_pair* d_pairs, const std::vector<uint64_t>& offs, size_t n, int len, u32 P,
                 const std::chrono::steady_clock::time_point* t_map, const vdjx_quant_params* prm, double* out_counts, vdjx_quant_info* info) {
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	HIP_TRY(hipStreamSynchronize(st));
	const double us_map = t_map ? q_us_since(*t_map) : 0.0;
	const u64 A64 = offs[n];
	u32 placed_contigs = 0;
	for (size_t i = 0; i < n; i++) placed_contigs += offs[i + 1] > offs[i] ? 1u : 0u;
	c->stats["quant_contigs_placed"] = placed_contigs;
	c->stats["quant_map_us"] = (uint64_t) us_map;
	c->stats["quant_setup_us"] = 0;
	c->stats["quant_em_us"] = 0;
	if (A64 == 0) {
		for (size_t i = 0; i < n; i++) out_counts[i] = 0.0;
		info->eff_len = q_eff_len_uniform(len);
		return VDJX_OK;
	}
	if (A64 >= (1ull << 32)) { vdjx_set_error("vdjx_quant: 2^32 placements or more"); return VDJX_ELIMIT; }
	const u32 A = (u32) A64;
	const auto t1 = std::chrono::steady_clock::now();

	// the M step's chunks: contig after contig, Q_CHUNK alignments at most
	std::vector<uint2> chunks;
	std::vector<u32> cstart(n + 1);
	for (size_t i = 0; i < n; i++) {
		cstart[i] = (u32) chunks.size();
		for (u64 b = offs[i]; b < offs[i + 1]; b += Q_CHUNK) chunks.push_back(make_uint2((u32) b, (u32) std::min<u64>(b + Q_CHUNK, offs[i + 1])));
	}
	cstart[n] = (u32) chunks.size();
	const u32 nch = (u32) chunks.size();

	u32 *d_deg, *d_seg, *d_tmp, *d_perm, *d_hist, *d_ct, *d_cstart;
	u64 *d_excl, *d_off;
	double *d_gtab, *d_g, *d_r, *d_N, *d_part;
	uint2* d_chunks;
	QState* d_st;
	HIP_TRY(db.alloc(&d_deg, (size_t) P + 1));
	HIP_TRY(db.alloc(&d_excl, (size_t) P + 1));
	HIP_TRY(db.alloc(&d_seg, (size_t) P + 1));
	HIP_TRY(db.alloc(&d_tmp, (size_t) A));
	HIP_TRY(db.alloc(&d_perm, (size_t) A));
	HIP_TRY(db.alloc(&d_hist, Q_NBINS));
	HIP_TRY(db.alloc(&d_gtab, Q_NBINS));
	HIP_TRY(db.alloc(&d_ct, (size_t) A));
	HIP_TRY(db.alloc(&d_g, (size_t) A));
	HIP_TRY(db.alloc(&d_r, (size_t) A));
	HIP_TRY(db.alloc(&d_off, n + 1));
	HIP_TRY(db.alloc(&d_N, 2 * n));
	HIP_TRY(db.alloc(&d_part, (size_t) nch));
	HIP_TRY(db.alloc(&d_chunks, (size_t) nch));
	HIP_TRY(db.alloc(&d_cstart, n + 1));
	HIP_TRY(db.alloc(&d_st, 1));
	HIP_TRY(hipMemcpyAsync(d_off, offs.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_chunks, chunks.data(), (size_t) nch * sizeof(uint2), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_cstart, cstart.data(), (n + 1) * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_deg, 0, (size_t) P * 4, st));
	HIP_TRY(hipMemsetAsync(d_hist, 0, Q_NBINS * 4, st));
	HIP_TRY(hipMemsetAsync(d_st, 0, sizeof(QState), st));
	const u32 gA = (A + 255) / 256, gP = (u32) (((u64) P + 255) / 256);
	{
		vdjx_prof_scope ps(c, "k_quant_setup");
		hipLaunchKernelGGL(k_q_degree, dim3(gA), dim3(256), 0, st, d_pairs, A, P, d_deg);
		{ const int rc_ = vdjx_scan_wide(db, st, (const u32*) d_deg, P, d_excl, q_deg_key()); if (rc_) return rc_; }
		hipLaunchKernelGGL(k_q_csr, dim3(gP ? gP : 1), dim3(256), 0, st, (const u32*) d_deg, (const u64*) d_excl, P, d_seg);
		hipLaunchKernelGGL(k_q_scatter, dim3(gA), dim3(256), 0, st, d_pairs, A, P, (const u64*) d_excl, d_deg, d_tmp);
	}
	u64 total = 0;
	HIP_TRY(hipMemcpyAsync(c->h_pin, d_excl + P, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	memcpy(&total, c->h_pin, 8);
	const u32 Pp = (u32) (total >> 32);
	if ((u32) total != A || Pp == 0) { vdjx_set_error("vdjx_quant: %u of %u placements name a pair of the read index", (u32) total, A); return VDJX_EHIP; }
	const u32 gPp = (Pp + 255) / 256;
	{
		vdjx_prof_scope ps(c, "k_quant_setup");
		hipLaunchKernelGGL(k_q_order, dim3(gPp), dim3(256), 0, st, (const u32*) d_seg, Pp, (const u32*) d_tmp, d_pairs, d_perm, d_hist);
		hipLaunchKernelGGL(k_q_gtab, dim3(1), dim3(64), 0, st, (const u32*) d_hist, len, d_gtab, d_st);
		hipLaunchKernelGGL(k_q_align, dim3(gA), dim3(256), 0, st, (const u32*) d_perm, A, d_pairs, (const u64*) d_off, (u32) n, (const double*) d_gtab, d_ct, d_g);
		hipLaunchKernelGGL(k_q_init, dim3((u32) ((n + 255) / 256)), dim3(256), 0, st, (const u64*) d_off, (u32) n, (double) Pp / (double) placed_contigs, d_N);
	}
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	const double us_setup = q_us_since(t1);
	const auto t2 = std::chrono::steady_clock::now();

	// iterations in batches: iteration t reads N[(t - 1) % 2] and writes N[t % 2]
	QState hs;
	memset(&hs, 0, sizeof hs);
	u32 queued = 0;
	while (!hs.done && queued < (u32) prm->max_iter) {
		const u32 upto = std::min<u32>(queued + Q_BATCH, (u32) prm->max_iter);
		{
			vdjx_prof_scope ps(c, "k_quant_em");
			for (u32 t = queued + 1; t <= upto; t++) {
				const double* Nold = d_N + (size_t) ((t - 1) & 1u) * n;
				double* Nnew = d_N + (size_t) (t & 1u) * n;
				hipLaunchKernelGGL(k_q_estep, dim3(gPp), dim3(256), 0, st, (const QState*) d_st, (const u32*) d_seg, Pp, (const u32*) d_ct, (const double*) d_g,
				                   (const u32*) d_perm, Nold, d_r);
				hipLaunchKernelGGL(k_q_mpart, dim3(nch), dim3(256), 0, st, (const QState*) d_st, (const uint2*) d_chunks, (const double*) d_r, d_part);
				hipLaunchKernelGGL(k_q_mfin, dim3(1), dim3(1024), 0, st, d_st, (u32) n, (const u32*) d_cstart, (const double*) d_part, Nold, Nnew, prm->tol,
				                   (u32) prm->max_iter);
			}
		}
		queued = upto;
		HIP_TRY(hipMemcpyAsync(c->h_pin, d_st, sizeof(QState), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(hipGetLastError());
		memcpy(&hs, c->h_pin, sizeof hs);
	}
	if (!hs.done || hs.iters < 1) { vdjx_set_error("vdjx_quant: the iterations did not end (%u of %d)", hs.iters, prm->max_iter); return VDJX_EHIP; }
	HIP_TRY(hipMemcpyAsync(out_counts, d_N + (size_t) (hs.iters & 1u) * n, n * sizeof(double), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	vdjx_prof_collect(c, false);
	c->stats["quant_setup_us"] = (uint64_t) us_setup;
	c->stats["quant_em_us"] = (uint64_t) q_us_since(t2);
	info->pairs = Pp;
	info->alignments = A;
	info->unique_pairs = hs.unique;
	info->iterations = hs.iters;
	info->converged = hs.delta < prm->tol ? 1u : 0u;
	info->eff_len = hs.eff_len;
	return VDJX_OK;
}

extern "C" int vdjx_quant(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_quant_params* prm, double* out_counts, vdjx_quant_info* info) {
	if (!c || !prm || !info || (n && (!contigs || !out_counts))) { vdjx_set_error("vdjx_quant: NULL argument"); return VDJX_EINVAL; }
	memset(info, 0, sizeof *info);
	if (prm->max_iter < 1) { vdjx_set_error("vdjx_quant: max_iter=%d must be at least 1", prm->max_iter); return VDJX_EINVAL; }
	if (!(prm->tol >= 0.0)) { vdjx_set_error("vdjx_quant: tol must be >= 0"); return VDJX_EINVAL; }
	info->converged = 1;
	if (n == 0) return VDJX_OK;
	if (len < 1) { vdjx_set_error("vdjx_quant: len=%d", len); return VDJX_EINVAL; }
	if (n >= (1ull << 20) || len >= 4096) { vdjx_set_error("vdjx_quant: at most 2^20 - 1 contigs of fewer than 4096 bases per call"); return VDJX_ELIMIT; }
	if (memchr(contigs, 0, n * (size_t) len)) { vdjx_set_error("vdjx_quant: contigs of unequal length (a NUL inside the %zu x %d characters)", n, len); return VDJX_EINVAL; }
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<uint64_t> offs(n + 1);
	const vdjx_pair* d_pairs = nullptr;
	int rc = vdjx_map_emit_device(c, contigs, n, len, offs.data(), &d_pairs);
	if (rc) return rc;
	vdjx_work db(c);
	return q_run(c, db, d_pairs, offs, n, len, c->n_pairs, &t0, prm, out_counts, info);
}

extern "C" int vdjx_quant_pairs(vdjx_ctx* c, const uint64_t* offsets, const vdjx_pair* pairs, size_t n, int len, uint32_t n_pairs,
                                const vdjx_quant_params* prm, double* out_counts, vdjx_quant_info* info) {
	if (!c || !prm || !info || (n && (!offsets || !out_counts))) { vdjx_set_error("vdjx_quant_pairs: NULL argument"); return VDJX_EINVAL; }
	memset(info, 0, sizeof *info);
	if (prm->max_iter < 1) { vdjx_set_error("vdjx_quant_pairs: max_iter=%d must be at least 1", prm->max_iter); return VDJX_EINVAL; }
	if (!(prm->tol >= 0.0)) { vdjx_set_error("vdjx_quant_pairs: tol must be >= 0"); return VDJX_EINVAL; }
	info->converged = 1;
	if (n == 0) return VDJX_OK;
	if (len < 1) { vdjx_set_error("vdjx_quant_pairs: len=%d", len); return VDJX_EINVAL; }
	if (n >= (1ull << 20) || len >= 4096) { vdjx_set_error("vdjx_quant_pairs: at most 2^20 - 1 contigs of fewer than 4096 bases per call"); return VDJX_ELIMIT; }
	if (offsets[0] != 0) { vdjx_set_error("vdjx_quant_pairs: offsets[0]=%llu must be 0", (unsigned long long) offsets[0]); return VDJX_EINVAL; }
	for (size_t i = 0; i < n; i++)
		if (offsets[i + 1] < offsets[i]) { vdjx_set_error("vdjx_quant_pairs: the offsets decrease at contig %zu", i); return VDJX_EINVAL; }
	const u64 A64 = offsets[n];
	if (A64 >= (1ull << 32)) { vdjx_set_error("vdjx_quant_pairs: 2^32 placements or more"); return VDJX_ELIMIT; }
	if (A64 && !pairs) { vdjx_set_error("vdjx_quant_pairs: NULL argument (pairs)"); return VDJX_EINVAL; }
	for (u64 a = 0; a < A64; a++)
		if (pairs[a].pair_id >= n_pairs) {
			vdjx_set_error("vdjx_quant_pairs: placement %llu names pair %u of %u", (unsigned long long) a, pairs[a].pair_id, n_pairs);
			return VDJX_EINVAL;
		}
	const std::vector<uint64_t> offs(offsets, offsets + n + 1);
	HIP_TRY(hipSetDevice(c->device));
	vdjx_work db(c);
	vdjx_pair* d_pairs = nullptr;
	if (A64) {
		HIP_TRY(db.alloc(&d_pairs, (size_t) A64));
		HIP_TRY(hipMemcpyAsync(d_pairs, pairs, (size_t) A64 * sizeof(vdjx_pair), hipMemcpyHostToDevice, c->stream));
	}
	return q_run(c, db, d_pairs, offs, n, len, n_pairs, nullptr, prm, out_counts, info);
}
