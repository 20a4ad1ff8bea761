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

// what q_setup builds once per call and both EMs read: the pair-major structure of the sample and the point estimate's buffers
struct QSetup {
	u32 A = 0, P = 0, Pp = 0, nch = 0, placed_contigs = 0;      // A == 0: no placement at all, nothing below is there
	u32 *d_seg = nullptr, *d_perm = nullptr, *d_ct = nullptr, *d_cstart = nullptr;
	u64 *d_excl = nullptr, *d_off = nullptr;
	double *d_g = nullptr, *d_r = nullptr, *d_N = nullptr, *d_part = nullptr;
	uint2* d_chunks = nullptr;
	QState* d_st = nullptr;
	double us_setup = 0.0;
};

// the structure over placements that are on the device already (contig-major, offs[n + 1] on the host).  t_map: when the caller began
// to map (nullptr: it did not, quant_map_us is 0)
static int q_setup(vdjx_ctx* c, vdjx_work& db, const vdjx_pair* d_pairs, const std::vector<uint64_t>& offs, size_t n, int len, u32 P,
                   const std::chrono::steady_clock::time_point* t_map, QSetup& s) {
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
	if (A64 == 0) return VDJX_OK;
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

	u32 *d_deg, *d_tmp, *d_hist;
	double* d_gtab;
	HIP_TRY(db.alloc(&d_deg, (size_t) P + 1));
	HIP_TRY(db.alloc(&s.d_excl, (size_t) P + 1));
	HIP_TRY(db.alloc(&s.d_seg, (size_t) P + 1));
	HIP_TRY(db.alloc(&d_tmp, (size_t) A));
	HIP_TRY(db.alloc(&s.d_perm, (size_t) A));
	HIP_TRY(db.alloc(&d_hist, Q_NBINS));
	HIP_TRY(db.alloc(&d_gtab, Q_NBINS));
	HIP_TRY(db.alloc(&s.d_ct, (size_t) A));
	HIP_TRY(db.alloc(&s.d_g, (size_t) A));
	HIP_TRY(db.alloc(&s.d_r, (size_t) A));
	HIP_TRY(db.alloc(&s.d_off, n + 1));
	HIP_TRY(db.alloc(&s.d_N, 2 * n));
	HIP_TRY(db.alloc(&s.d_part, (size_t) nch));
	HIP_TRY(db.alloc(&s.d_chunks, (size_t) nch));
	HIP_TRY(db.alloc(&s.d_cstart, n + 1));
	HIP_TRY(db.alloc(&s.d_st, 1));
	HIP_TRY(hipMemcpyAsync(s.d_off, offs.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(s.d_chunks, chunks.data(), (size_t) nch * sizeof(uint2), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(s.d_cstart, cstart.data(), (n + 1) * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_deg, 0, (size_t) P * 4, st));
	HIP_TRY(hipMemsetAsync(d_hist, 0, Q_NBINS * 4, st));
	HIP_TRY(hipMemsetAsync(s.d_st, 0, sizeof(QState), st));
	const u32 gA = (A + 255) / 256, gP = (u32) (((u64) P + 255) / 256);
	{
		vdjx_prof_scope ps(c, "k_quant_setup");
		hipLaunchKernelGGL(k_q_degree, dim3(gA), dim3(256), 0, st, d_pairs, A, P, d_deg);
		{ const int rc_ = vdjx_scan_wide(db, st, (const u32*) d_deg, P, s.d_excl, q_deg_key()); if (rc_) return rc_; }
		hipLaunchKernelGGL(k_q_csr, dim3(gP ? gP : 1), dim3(256), 0, st, (const u32*) d_deg, (const u64*) s.d_excl, P, s.d_seg);
		hipLaunchKernelGGL(k_q_scatter, dim3(gA), dim3(256), 0, st, d_pairs, A, P, (const u64*) s.d_excl, d_deg, d_tmp);
	}
	u64 total = 0;
	HIP_TRY(hipMemcpyAsync(c->h_pin, s.d_excl + P, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	memcpy(&total, c->h_pin, 8);
	const u32 Pp = (u32) (total >> 32);
	if ((u32) total != A || Pp == 0) { vdjx_set_error("vdjx_quant: %u of %u placements name a pair of the read index", (u32) total, A); return VDJX_EHIP; }
	const u32 gPp = (Pp + 255) / 256;
	{
		vdjx_prof_scope ps(c, "k_quant_setup");
		hipLaunchKernelGGL(k_q_order, dim3(gPp), dim3(256), 0, st, (const u32*) s.d_seg, Pp, (const u32*) d_tmp, d_pairs, s.d_perm, d_hist);
		hipLaunchKernelGGL(k_q_gtab, dim3(1), dim3(64), 0, st, (const u32*) d_hist, len, d_gtab, s.d_st);
		hipLaunchKernelGGL(k_q_align, dim3(gA), dim3(256), 0, st, (const u32*) s.d_perm, A, d_pairs, (const u64*) s.d_off, (u32) n, (const double*) d_gtab, s.d_ct, s.d_g);
		hipLaunchKernelGGL(k_q_init, dim3((u32) ((n + 255) / 256)), dim3(256), 0, st, (const u64*) s.d_off, (u32) n, (double) Pp / (double) placed_contigs, s.d_N);
	}
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	s.A = A;
	s.P = P;
	s.Pp = Pp;
	s.nch = nch;
	s.placed_contigs = placed_contigs;
	s.us_setup = q_us_since(t1);
	return VDJX_OK;
}

// the point estimate's EM over q_setup's structure
static int q_em(vdjx_ctx* c, const QSetup& s, size_t n, const vdjx_quant_params* prm, double* out_counts, vdjx_quant_info* info) {
	hipStream_t st = c->stream;
	const u32 gPp = (s.Pp + 255) / 256;
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
				const double* Nold = s.d_N + (size_t) ((t - 1) & 1u) * n;
				double* Nnew = s.d_N + (size_t) (t & 1u) * n;
				hipLaunchKernelGGL(k_q_estep, dim3(gPp), dim3(256), 0, st, (const QState*) s.d_st, (const u32*) s.d_seg, s.Pp, (const u32*) s.d_ct, (const double*) s.d_g,
				                   (const u32*) s.d_perm, Nold, s.d_r);
				hipLaunchKernelGGL(k_q_mpart, dim3(s.nch), dim3(256), 0, st, (const QState*) s.d_st, (const uint2*) s.d_chunks, (const double*) s.d_r, s.d_part);
				hipLaunchKernelGGL(k_q_mfin, dim3(1), dim3(1024), 0, st, s.d_st, (u32) n, (const u32*) s.d_cstart, (const double*) s.d_part, Nold, Nnew, prm->tol,
				                   (u32) prm->max_iter);
			}
		}
		queued = upto;
		HIP_TRY(hipMemcpyAsync(c->h_pin, s.d_st, sizeof(QState), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(hipGetLastError());
		memcpy(&hs, c->h_pin, sizeof hs);
	}
	if (!hs.done || hs.iters < 1) { vdjx_set_error("vdjx_quant: the iterations did not end (%u of %d)", hs.iters, prm->max_iter); return VDJX_EHIP; }
	HIP_TRY(hipMemcpyAsync(out_counts, s.d_N + (size_t) (hs.iters & 1u) * n, n * sizeof(double), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	vdjx_prof_collect(c, false);
	c->stats["quant_setup_us"] = (uint64_t) s.us_setup;
	c->stats["quant_em_us"] = (uint64_t) q_us_since(t2);
	info->pairs = s.Pp;
	info->alignments = s.A;
	info->unique_pairs = hs.unique;
	info->iterations = hs.iters;
	info->converged = hs.delta < prm->tol ? 1u : 0u;
	info->eff_len = hs.eff_len;
	return VDJX_OK;
}

// ---- the bootstrap: B replicates of the EM over the same structure, each with a multiplicity per placed pair --------------------------
// Layout: the replicate is innermost.  m[q][b] (uint32) and sum[q][b] (the E step's sum over pair q) for the placed pairs, N[c][b] twice
// (iteration t reads buffer (t - 1) & 1 and writes t & 1), part[k][b] for the M step's chunks; b = 0 .. Bb - 1 are the replicates of
// one batch.  A wave therefore reads an alignment's pair, contig and g once (one address for all lanes) and carries up to 64
// replicates in its lanes, whose own values lie side by side.  Every sum is made in an order that the number of replicates in the
// batch does not enter: a replicate has the same bits in any batch.
//   k_qb_draw   one dispatch per batch: draw i of replicate r on slot hi64(mix64(mix64(seed) + (r << 32 | i)) * Pp), integer atomics
//   k_qb_esum   a thread per (pair, replicate): sum = the pair's N_c g in slot order (r itself is never stored)
//   k_qb_mpart  a workgroup per (chunk of QB_CHUNK alignments of one contig, tile of T replicates): the chunk in QB_SLICES slices of
//               QB_SLICE alignments, a thread sums a slice's m (w / sum) in order, then the slices are added in order
//   k_qb_mfin   a thread per (contig, replicate): its chunks in order, the stop rule's term; the maximum per replicate through LDS and
//               one integer atomicMax on the bits of the (non-negative) double
//   k_qb_stop   one workgroup: counts the iteration of every live replicate, sets its flag, counts the finished ones
// A finished replicate's threads return at once; a batch whose replicates are all finished makes every kernel return at entry.
#define QB_CHUNK 512u
#define QB_SLICE 16u
#define QB_SLICES (QB_CHUNK / QB_SLICE)
#define QB_FIN_PER 8u                    // contigs a thread of k_qb_mfin takes

struct QBState {
	u32 done, iters;
	double delta;
};

// per alignment in contig-major order: its pair's slot and its g (the inverse of perm)
__global__ void k_qb_inverse(const u32* __restrict__ seg, u32 Pp, const u32* __restrict__ perm, const double* __restrict__ g, u32* __restrict__ aq,
                             double* __restrict__ ag) {
	const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= Pp) return;
	const u32 e = seg[q + 1];
	for (u32 j = seg[q]; j < e; j++) {
		const u32 a = perm[j];
		aq[a] = q;
		ag[a] = g[j];
	}
}

__global__ void k_qb_init(const u64* __restrict__ off, u32 n, u32 Bb, double v, double* __restrict__ N) {
	const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n * Bb) return;
	const u32 c = t / Bb;
	N[t] = off[c + 1] > off[c] ? v : 0.0;
}

// m is zero; replicate r = r0 + b + 1
__global__ void k_qb_draw(u32 Pp, u32 Bb, u32 r0, u64 seedmix, u32* __restrict__ m) {
	const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= Pp * Bb) return;
	const u32 b = t % Bb;
	const u64 i = t / Bb, r = (u64) r0 + b + 1u;
	const u64 slot = __umul64hi(vdjx_mix64(seedmix + (r << 32 | i)), (u64) Pp);      // < Pp
	atomicAdd(&m[slot * Bb + b], 1u);
}

// the caller's multiplicities (src[b][p], by pair id) into m, or m out to dst[b][p] (0 for an id without a placement).  A placed id's
// slot is the high word of its exclusive prefix, which the next id's exceeds by one
template <bool OUT>
__global__ void k_qb_mult(const u64* __restrict__ excl, u32 P, u32 Bb, u32* __restrict__ m, u32* __restrict__ ext) {
	const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= P * Bb) return;
	const u32 p = t % P, b = t / P;
	const u32 q = (u32) (excl[p] >> 32);
	const bool placed = (u32) (excl[p + 1] >> 32) != q;
	if (OUT) ext[t] = placed ? m[(size_t) q * Bb + b] : 0u;
	else if (placed) m[(size_t) q * Bb + b] = ext[t];
}

__global__ __launch_bounds__(256) void k_qb_esum(const u32* __restrict__ ndone, const QBState* __restrict__ st, const u32* __restrict__ seg, u32 Pp, u32 Bb,
                                                 const u32* __restrict__ ct, const double* __restrict__ g, const double* __restrict__ N,
                                                 double* __restrict__ sum) {
	if (*ndone == Bb) return;
	const u32 t = blockIdx.x * 256u + threadIdx.x;
	if (t >= Pp * Bb) return;
	const u32 b = t % Bb, q = t / Bb;
	if (st[b].done) return;
	const u32 e = seg[q + 1];
	double s = 0.0;
	for (u32 j = seg[q]; j < e; j++) s += N[(size_t) ct[j] * Bb + b] * g[j];
	sum[t] = s;
}

// T: the tile's width, a power of two <= 64; thread (grp, bl) = (threadIdx.x / T, threadIdx.x % T), replicate blockIdx.y * T + bl
__global__ __launch_bounds__(256) void k_qb_mpart(const u32* __restrict__ ndone, const QBState* __restrict__ st, const uint2* __restrict__ chunks,
                                                  const u32* __restrict__ cc, u32 Bb, u32 T, const u32* __restrict__ aq, const double* __restrict__ ag,
                                                  const double* __restrict__ N, const double* __restrict__ sum, const u32* __restrict__ m,
                                                  double* __restrict__ part) {
	__shared__ double sl[QB_SLICES * 64u];
	if (*ndone == Bb) return;
	const uint2 ch = chunks[blockIdx.x];
	const u32 bl = threadIdx.x & (T - 1u), grp = threadIdx.x / T, G = 256u / T;
	const u32 b = blockIdx.y * T + bl;
	const bool live = b < Bb && !st[b].done;
	if (live) {
		const double Nc = N[(size_t) cc[blockIdx.x] * Bb + b];
		const u32 len = ch.y - ch.x;
		for (u32 s = grp; s < QB_SLICES; s += G) {
			const u32 lo = min(s * QB_SLICE, len), hi = min(lo + QB_SLICE, len);
			double v = 0.0;
			for (u32 a = ch.x + lo; a < ch.x + hi; a++) {
				const size_t k = (size_t) aq[a] * Bb + b;
				const double w = Nc * ag[a], sm = sum[k];
				if (sm > 0.0) v += (double) m[k] * (w / sm);
			}
			sl[s * T + bl] = v;
		}
	}
	__syncthreads();
	if (live && grp == 0) {
		double v = 0.0;
		for (u32 s = 0; s < QB_SLICES; s++) v += sl[s * T + bl];
		part[(size_t) blockIdx.x * Bb + b] = v;
	}
}

__global__ __launch_bounds__(256) void k_qb_mfin(const u32* __restrict__ ndone, const QBState* __restrict__ st, u32 n, u32 Bb, u32 T,
                                                 const u32* __restrict__ cstart, const double* __restrict__ part, const double* __restrict__ Nold,
                                                 double* __restrict__ Nnew, unsigned long long* __restrict__ dmax) {
	__shared__ double sm[256];
	if (*ndone == Bb) return;
	const u32 bl = threadIdx.x & (T - 1u), grp = threadIdx.x / T, G = 256u / T;
	const u32 b = blockIdx.y * T + bl;
	const bool live = b < Bb && !st[b].done;
	double mx = 0.0;
	if (live)
		for (u32 i = 0; i < QB_FIN_PER; i++) {
			const u32 c = (blockIdx.x * QB_FIN_PER + i) * G + grp;
			if (c >= n) break;
			const u32 e = cstart[c + 1];
			double v = 0.0;
			for (u32 k = cstart[c]; k < e; k++) v += part[(size_t) k * Bb + b];
			const size_t at = (size_t) c * Bb + b;
			Nnew[at] = v;
			mx = fmax(mx, fabs(v - Nold[at]) / fmax(v, 1.0));
		}
	sm[threadIdx.x] = mx;
	__syncthreads();
	if (live && grp == 0) {
		for (u32 k = 1; k < G; k++) mx = fmax(mx, sm[k * T + bl]);
		// (the bits of a non-negative double order like the double: an integer maximum, whatever order the workgroups come in)
		if (mx > 0.0) atomicMax(&dmax[b], (unsigned long long) __double_as_longlong(mx));
	}
}

__global__ __launch_bounds__(256) void k_qb_stop(u32* __restrict__ ndone, QBState* __restrict__ st, u32 Bb, unsigned long long* __restrict__ dmax, double tol,
                                                 u32 max_iter) {
	__shared__ u32 cnt;
	const bool over = *ndone == Bb;
	if (threadIdx.x == 0) cnt = 0;
	__syncthreads();
	if (over) return;
	u32 mine = 0;
	for (u32 b = threadIdx.x; b < Bb; b += 256u) {
		u32 done = st[b].done;
		if (!done) {
			const u32 it = st[b].iters + 1u;
			const double d = __longlong_as_double((long long) dmax[b]);
			dmax[b] = 0ull;
			st[b].iters = it;
			st[b].delta = d;
			done = (d < tol || it >= max_iter) ? 1u : 0u;
			st[b].done = done;
		}
		mine += done;
	}
	if (mine) atomicAdd(&cnt, mine);
	__syncthreads();
	if (threadIdx.x == 0) *ndone = cnt;
}

// replicate-major out of the buffer every replicate's last iteration wrote
__global__ void k_qb_out(const QBState* __restrict__ st, u32 n, u32 Bb, const double* __restrict__ N, double* __restrict__ out, u32* __restrict__ iters) {
	const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n * Bb) return;
	const u32 b = t % Bb, c = t / Bb;
	const u32 it = st[b].iters;
	out[(size_t) b * n + c] = N[(size_t) (it & 1u) * n * Bb + t];
	if (c == 0) iters[b] = it;
}

// the bootstrap over q_setup's structure (s.A > 0).  mult / out_mult: NULL or B x P by pair id (vdjx_quant_pairs_boot)
static int qb_run(vdjx_ctx* c, vdjx_work& db, const QSetup& s, const std::vector<uint64_t>& offs, size_t n, const vdjx_quant_params* prm,
                  const vdjx_quant_boot_params* bp, const u32* mult, u32* out_mult, double* out_boot, u32* out_iters, vdjx_quant_boot_info* binfo) {
	hipStream_t st = c->stream;
	const auto t0 = std::chrono::steady_clock::now();
	const u32 B = (u32) bp->replicates, Pp = s.Pp, P = s.P, nn = (u32) n;
	// a replicate takes Pp + n cells (its multiplicities and pair sums, its counts); no index of a batch reaches 2^32
	const u64 cells = (u64) vdjx_env_num("VDJX_QBOOT_CELLS", 1ll << 30, 1, 1ll << 32);
	u64 fit = std::max<u64>(1, cells / ((u64) Pp + n));
	fit = std::min<u64>(fit, 0xFFFFFFFFull / std::max<u64>(Pp, n));
	if (mult || out_mult) fit = std::min<u64>(fit, 0xFFFFFFFFull / P);
	const u32 per_batch = (u32) std::min<u64>(B, std::max<u64>(1, fit));

	// the M step's chunks of QB_CHUNK alignments, contig after contig, and the contig of every chunk
	std::vector<uint2> chunks;
	std::vector<u32> cstart(n + 1), cc;
	for (size_t i = 0; i < n; i++) {
		cstart[i] = (u32) chunks.size();
		for (u64 b = offs[i]; b < offs[i + 1]; b += QB_CHUNK) {
			chunks.push_back(make_uint2((u32) b, (u32) std::min<u64>(b + QB_CHUNK, offs[i + 1])));
			cc.push_back((u32) i);
		}
	}
	cstart[n] = (u32) chunks.size();
	const u32 nch = (u32) chunks.size();

	u32 *d_aq, *d_cc, *d_cstart, *d_m, *d_ndone, *d_iters, *d_ext = nullptr;
	double *d_ag, *d_sum, *d_N, *d_part, *d_out;
	uint2* d_chunks;
	QBState* d_st;
	unsigned long long* d_dmax;
	HIP_TRY(db.alloc(&d_aq, (size_t) s.A));
	HIP_TRY(db.alloc(&d_ag, (size_t) s.A));
	HIP_TRY(db.alloc(&d_chunks, (size_t) nch));
	HIP_TRY(db.alloc(&d_cc, (size_t) nch));
	HIP_TRY(db.alloc(&d_cstart, n + 1));
	HIP_TRY(db.alloc(&d_m, (size_t) Pp * per_batch));
	HIP_TRY(db.alloc(&d_sum, (size_t) Pp * per_batch));
	HIP_TRY(db.alloc(&d_N, 2 * n * per_batch));
	HIP_TRY(db.alloc(&d_part, (size_t) nch * per_batch));
	HIP_TRY(db.alloc(&d_out, n * per_batch));
	HIP_TRY(db.alloc(&d_st, (size_t) per_batch));
	HIP_TRY(db.alloc(&d_dmax, (size_t) per_batch));
	HIP_TRY(db.alloc(&d_iters, (size_t) per_batch));
	HIP_TRY(db.alloc(&d_ndone, 1));
	if (mult || out_mult) HIP_TRY(db.alloc(&d_ext, (size_t) P * per_batch));
	HIP_TRY(hipMemcpyAsync(d_chunks, chunks.data(), (size_t) nch * sizeof(uint2), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_cc, cc.data(), (size_t) nch * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_cstart, cstart.data(), (n + 1) * 4, hipMemcpyHostToDevice, st));
	{
		vdjx_prof_scope ps(c, "k_quant_boot_setup");
		hipLaunchKernelGGL(k_qb_inverse, dim3((Pp + 255) / 256), dim3(256), 0, st, (const u32*) s.d_seg, Pp, (const u32*) s.d_perm, (const double*) s.d_g, d_aq, d_ag);
	}
	const u64 seedmix = vdjx_mix64(bp->seed);
	const double start = (double) Pp / (double) s.placed_contigs;
	std::vector<QBState> hst(per_batch);
	vdjx_quant_boot_info inf;
	memset(&inf, 0, sizeof inf);
	inf.replicates = B;
	double us_em = 0.0;
	for (u32 r0 = 0; r0 < B; r0 += per_batch) {
		const u32 Bb = std::min(per_batch, B - r0);
		u32 T = 1;
		while (T < 64u && T < Bb) T <<= 1;
		const u32 tiles = (Bb + T - 1) / T, G = 256u / T;
		const u32 gPB = (u32) (((u64) Pp * Bb + 255) / 256), gNB = (u32) (((u64) nn * Bb + 255) / 256);
		HIP_TRY(hipMemsetAsync(d_m, 0, (size_t) Pp * Bb * 4, st));
		HIP_TRY(hipMemsetAsync(d_st, 0, (size_t) Bb * sizeof(QBState), st));
		HIP_TRY(hipMemsetAsync(d_dmax, 0, (size_t) Bb * 8, st));
		HIP_TRY(hipMemsetAsync(d_ndone, 0, 4, st));
		if (mult) {
			HIP_TRY(hipMemcpyAsync(d_ext, mult + (size_t) r0 * P, (size_t) Bb * P * 4, hipMemcpyHostToDevice, st));
			vdjx_prof_scope ps(c, "k_quant_boot_draw");
			hipLaunchKernelGGL(k_qb_mult<false>, dim3((u32) (((u64) P * Bb + 255) / 256)), dim3(256), 0, st, (const u64*) s.d_excl, P, Bb, d_m, d_ext);
		} else {
			vdjx_prof_scope ps(c, "k_quant_boot_draw");
			hipLaunchKernelGGL(k_qb_draw, dim3(gPB), dim3(256), 0, st, Pp, Bb, r0, seedmix, d_m);
		}
		if (out_mult) {
			hipLaunchKernelGGL(k_qb_mult<true>, dim3((u32) (((u64) P * Bb + 255) / 256)), dim3(256), 0, st, (const u64*) s.d_excl, P, Bb, d_m, d_ext);
			HIP_TRY(hipMemcpyAsync(out_mult + (size_t) r0 * P, d_ext, (size_t) Bb * P * 4, hipMemcpyDeviceToHost, st));
		}
		hipLaunchKernelGGL(k_qb_init, dim3(gNB), dim3(256), 0, st, (const u64*) s.d_off, nn, Bb, start, d_N);
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(hipGetLastError());
		const auto t1 = std::chrono::steady_clock::now();
		u32 ndone = 0, queued = 0;
		while (ndone < Bb && queued < (u32) prm->max_iter) {
			const u32 upto = std::min<u32>(queued + Q_BATCH, (u32) prm->max_iter);
			{
				vdjx_prof_scope ps(c, "k_quant_boot_em");
				for (u32 t = queued + 1; t <= upto; t++) {
					const double* Nold = d_N + (size_t) ((t - 1) & 1u) * n * Bb;
					double* Nnew = d_N + (size_t) (t & 1u) * n * Bb;
					hipLaunchKernelGGL(k_qb_esum, dim3(gPB), dim3(256), 0, st, (const u32*) d_ndone, (const QBState*) d_st, (const u32*) s.d_seg, Pp, Bb,
					                   (const u32*) s.d_ct, (const double*) s.d_g, Nold, d_sum);
					hipLaunchKernelGGL(k_qb_mpart, dim3(nch, tiles), dim3(256), 0, st, (const u32*) d_ndone, (const QBState*) d_st, (const uint2*) d_chunks,
					                   (const u32*) d_cc, Bb, T, (const u32*) d_aq, (const double*) d_ag, Nold, (const double*) d_sum, (const u32*) d_m, d_part);
					hipLaunchKernelGGL(k_qb_mfin, dim3((nn + G * QB_FIN_PER - 1) / (G * QB_FIN_PER), tiles), dim3(256), 0, st, (const u32*) d_ndone,
					                   (const QBState*) d_st, nn, Bb, T, (const u32*) d_cstart, (const double*) d_part, Nold, Nnew, d_dmax);
					hipLaunchKernelGGL(k_qb_stop, dim3(1), dim3(256), 0, st, d_ndone, d_st, Bb, d_dmax, prm->tol, (u32) prm->max_iter);
				}
			}
			queued = upto;
			HIP_TRY(hipMemcpyAsync(c->h_pin, d_ndone, 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			HIP_TRY(hipGetLastError());
			memcpy(&ndone, c->h_pin, 4);
		}
		if (ndone != Bb) { vdjx_set_error("vdjx_quant_boot: the iterations did not end (%u of %u replicates, %d iterations)", ndone, Bb, prm->max_iter); return VDJX_EHIP; }
		us_em += q_us_since(t1);
		hipLaunchKernelGGL(k_qb_out, dim3(gNB), dim3(256), 0, st, (const QBState*) d_st, nn, Bb, (const double*) d_N, d_out, d_iters);
		HIP_TRY(hipMemcpyAsync(out_boot + (size_t) r0 * n, d_out, (size_t) Bb * n * sizeof(double), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(out_iters + r0, d_iters, (size_t) Bb * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(hst.data(), d_st, (size_t) Bb * sizeof(QBState), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(hipGetLastError());
		vdjx_prof_collect(c, false);
		for (u32 b = 0; b < Bb; b++) {
			inf.converged += hst[b].delta < prm->tol ? 1u : 0u;
			inf.iterations += hst[b].iters;
			inf.max_iterations = std::max(inf.max_iterations, hst[b].iters);
		}
		inf.batches++;
	}
	*binfo = inf;
	c->stats["quant_boot_em_us"] = (uint64_t) us_em;
	c->stats["quant_boot_us"] = (uint64_t) q_us_since(t0);
	return VDJX_OK;
}

// what an empty call gives: zeros, no iteration, every replicate converged
static void qb_empty(size_t n, const vdjx_quant_boot_params* bp, double* out_boot, u32* out_iters, vdjx_quant_boot_info* binfo) {
	const u32 B = (u32) bp->replicates;
	for (size_t i = 0; i < (size_t) B * n; i++) out_boot[i] = 0.0;
	for (u32 r = 0; r < B; r++) out_iters[r] = 0;
	binfo->replicates = B;
	binfo->converged = B;
}

// the bootstrap's own arguments (bp == nullptr: the call has no bootstrap)
static int qb_check(const char* who, size_t n, const vdjx_quant_boot_params* bp, const double* out_boot, const u32* out_iters, const vdjx_quant_boot_info* binfo) {
	if (!bp || !out_iters || !binfo || (n && !out_boot)) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	if (bp->replicates < 1 || bp->replicates > 1024) { vdjx_set_error("%s: %d replicates (1 .. 1024)", who, bp->replicates); return VDJX_EINVAL; }
	return VDJX_OK;
}

static int q_contigs(const char* who, bool boot, vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_quant_params* prm,
                     const vdjx_quant_boot_params* bp, double* out_counts, vdjx_quant_info* info, double* out_boot, u32* out_iters,
                     vdjx_quant_boot_info* binfo) {
	if (!c || !prm || !info || (n && (!contigs || !out_counts))) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	memset(info, 0, sizeof *info);
	if (boot) {
		const int rc = qb_check(who, n, bp, out_boot, out_iters, binfo);
		if (rc) return rc;
		memset(binfo, 0, sizeof *binfo);
	}
	if (prm->max_iter < 1) { vdjx_set_error("%s: max_iter=%d must be at least 1", who, prm->max_iter); return VDJX_EINVAL; }
	if (!(prm->tol >= 0.0)) { vdjx_set_error("%s: tol must be >= 0", who); return VDJX_EINVAL; }
	info->converged = 1;
	if (boot) qb_empty(0, bp, out_boot, out_iters, binfo);
	if (n == 0) return VDJX_OK;
	if (len < 1) { vdjx_set_error("%s: len=%d", who, len); return VDJX_EINVAL; }
	if (n >= (1ull << 20) || len >= 4096) { vdjx_set_error("%s: at most 2^20 - 1 contigs of fewer than 4096 bases per call", who); return VDJX_ELIMIT; }
	if (boot && (u64) bp->replicates * n >= (1ull << 27)) { vdjx_set_error("%s: %d replicates x %zu contigs (fewer than 2^27 counts per call)", who, bp->replicates, n); return VDJX_ELIMIT; }
	if (memchr(contigs, 0, n * (size_t) len)) { vdjx_set_error("%s: contigs of unequal length (a NUL inside the %zu x %d characters)", who, n, len); return VDJX_EINVAL; }
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<uint64_t> offs(n + 1);
	const vdjx_pair* d_pairs = nullptr;
	int rc = vdjx_map_emit_device(c, contigs, n, len, offs.data(), &d_pairs);
	if (rc) return rc;
	vdjx_work db(c);
	QSetup s;
	rc = q_setup(c, db, d_pairs, offs, n, len, c->n_pairs, &t0, s);
	if (rc) return rc;
	if (s.A == 0) {
		for (size_t i = 0; i < n; i++) out_counts[i] = 0.0;
		info->eff_len = q_eff_len_uniform(len);
		if (boot) qb_empty(n, bp, out_boot, out_iters, binfo);
		return VDJX_OK;
	}
	rc = q_em(c, s, n, prm, out_counts, info);
	if (rc || !boot) return rc;
	return qb_run(c, db, s, offs, n, prm, bp, nullptr, nullptr, out_boot, out_iters, binfo);
}

extern "C" int vdjx_quant(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_quant_params* prm, double* out_counts, vdjx_quant_info* info) {
	return q_contigs("vdjx_quant", false, c, contigs, n, len, prm, nullptr, out_counts, info, nullptr, nullptr, nullptr);
}

extern "C" int vdjx_quant_boot(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_quant_params* prm, const vdjx_quant_boot_params* bp,
                               double* out_counts, vdjx_quant_info* info, double* out_boot, uint32_t* out_iters, vdjx_quant_boot_info* binfo) {
	return q_contigs("vdjx_quant_boot", true, c, contigs, n, len, prm, bp, out_counts, info, out_boot, out_iters, binfo);
}

static int q_placements(const char* who, bool boot, vdjx_ctx* c, const uint64_t* offsets, const vdjx_pair* pairs, size_t n, int len, uint32_t n_pairs,
                        const vdjx_quant_params* prm, const vdjx_quant_boot_params* bp, const u32* mult, u32* out_mult, double* out_counts,
                        vdjx_quant_info* info, double* out_boot, u32* out_iters, vdjx_quant_boot_info* binfo) {
	if (!c || !prm || !info || (n && (!offsets || !out_counts))) { vdjx_set_error("%s: NULL argument", who); return VDJX_EINVAL; }
	memset(info, 0, sizeof *info);
	if (boot) {
		const int rc = qb_check(who, n, bp, out_boot, out_iters, binfo);
		if (rc) return rc;
		memset(binfo, 0, sizeof *binfo);
	}
	if (prm->max_iter < 1) { vdjx_set_error("%s: max_iter=%d must be at least 1", who, prm->max_iter); return VDJX_EINVAL; }
	if (!(prm->tol >= 0.0)) { vdjx_set_error("%s: tol must be >= 0", who); return VDJX_EINVAL; }
	info->converged = 1;
	const size_t BP = boot ? (size_t) bp->replicates * n_pairs : 0;
	if (boot) {
		qb_empty(0, bp, out_boot, out_iters, binfo);
		if (out_mult) memset(out_mult, 0, BP * 4);
	}
	if (n == 0) return VDJX_OK;
	if (len < 1) { vdjx_set_error("%s: len=%d", who, len); return VDJX_EINVAL; }
	if (n >= (1ull << 20) || len >= 4096) { vdjx_set_error("%s: at most 2^20 - 1 contigs of fewer than 4096 bases per call", who); return VDJX_ELIMIT; }
	if (boot && (u64) bp->replicates * n >= (1ull << 27)) { vdjx_set_error("%s: %d replicates x %zu contigs (fewer than 2^27 counts per call)", who, bp->replicates, n); return VDJX_ELIMIT; }
	if (offsets[0] != 0) { vdjx_set_error("%s: offsets[0]=%llu must be 0", who, (unsigned long long) offsets[0]); return VDJX_EINVAL; }
	for (size_t i = 0; i < n; i++)
		if (offsets[i + 1] < offsets[i]) { vdjx_set_error("%s: the offsets decrease at contig %zu", who, i); return VDJX_EINVAL; }
	const u64 A64 = offsets[n];
	if (A64 >= (1ull << 32)) { vdjx_set_error("%s: 2^32 placements or more", who); return VDJX_ELIMIT; }
	if (A64 && !pairs) { vdjx_set_error("%s: NULL argument (pairs)", who); return VDJX_EINVAL; }
	for (u64 a = 0; a < A64; a++)
		if (pairs[a].pair_id >= n_pairs) {
			vdjx_set_error("%s: placement %llu names pair %u of %u", who, (unsigned long long) a, pairs[a].pair_id, n_pairs);
			return VDJX_EINVAL;
		}
	if (boot && mult && A64) {                 // a replicate's multiplicities over the placed ids, before any GPU work
		std::vector<bool> placed(n_pairs, false);
		for (u64 a = 0; a < A64; a++) placed[pairs[a].pair_id] = true;
		for (int r = 0; r < bp->replicates; r++) {
			u64 tot = 0;
			for (u32 p = 0; p < n_pairs; p++)
				if (placed[p]) tot += mult[(size_t) r * n_pairs + p];
			if (tot >= (1ull << 32)) { vdjx_set_error("%s: the multiplicities of replicate %d sum to %llu (below 2^32)", who, r + 1, (unsigned long long) tot); return VDJX_EINVAL; }
		}
	}
	const std::vector<uint64_t> offs(offsets, offsets + n + 1);
	HIP_TRY(hipSetDevice(c->device));
	vdjx_work db(c);
	vdjx_pair* d_pairs = nullptr;
	if (A64) {
		HIP_TRY(db.alloc(&d_pairs, (size_t) A64));
		HIP_TRY(hipMemcpyAsync(d_pairs, pairs, (size_t) A64 * sizeof(vdjx_pair), hipMemcpyHostToDevice, c->stream));
	}
	QSetup s;
	int rc = q_setup(c, db, d_pairs, offs, n, len, n_pairs, nullptr, s);
	if (rc) return rc;
	if (s.A == 0) {
		for (size_t i = 0; i < n; i++) out_counts[i] = 0.0;
		info->eff_len = q_eff_len_uniform(len);
		if (boot) qb_empty(n, bp, out_boot, out_iters, binfo);
		return VDJX_OK;
	}
	rc = q_em(c, s, n, prm, out_counts, info);
	if (rc || !boot) return rc;
	return qb_run(c, db, s, offs, n, prm, bp, mult, out_mult, out_boot, out_iters, binfo);
}

extern "C" int vdjx_quant_pairs(vdjx_ctx* c, const uint64_t* offsets, const vdjx_pair* pairs, size_t n, int len, uint32_t n_pairs,
                                const vdjx_quant_params* prm, double* out_counts, vdjx_quant_info* info) {
	return q_placements("vdjx_quant_pairs", false, c, offsets, pairs, n, len, n_pairs, prm, nullptr, nullptr, nullptr, out_counts, info, nullptr, nullptr, nullptr);
}

extern "C" int vdjx_quant_pairs_boot(vdjx_ctx* c, const uint64_t* offsets, const vdjx_pair* pairs, size_t n, int len, uint32_t n_pairs,
                                     const vdjx_quant_params* prm, const vdjx_quant_boot_params* bp, const uint32_t* mult, uint32_t* out_mult,
                                     double* out_counts, vdjx_quant_info* info, double* out_boot, uint32_t* out_iters, vdjx_quant_boot_info* binfo) {
	return q_placements("vdjx_quant_pairs_boot", true, c, offsets, pairs, n, len, n_pairs, prm, bp, mult, out_mult, out_counts, info, out_boot, out_iters, binfo);
}

// plain C, no GPU: per contig the mean and sd (n - 1) of the replicates in replicate order, and the 2.5 % and 97.5 % order statistics
extern "C" void vdjx_quant_boot_summary(const double* boot, uint32_t B, size_t n, double* mean, double* sd, double* lower, double* upper) {
	if (!boot || B < 1) return;
	const size_t lo = (size_t) (25ull * (B - 1) / 1000ull), hi = (size_t) ((975ull * (B - 1) + 999ull) / 1000ull);
	std::vector<double> v(B);
	for (size_t c = 0; c < n; c++) {
		double s = 0.0, e2 = 0.0;
		for (u32 r = 0; r < B; r++) s += (v[r] = boot[(size_t) r * n + c]);
		const double mu = s / (double) B;
		for (u32 r = 0; r < B; r++) {
			const double e = v[r] - mu;
			e2 += e * e;
		}
		std::sort(v.begin(), v.end());
		if (mean) mean[c] = mu;
		if (sd) sd[c] = B > 1 ? sqrt(e2 / (double) (B - 1)) : 0.0;
		if (lower) lower[c] = v[lo];
		if (upper) upper[c] = v[hi];
	}
}
