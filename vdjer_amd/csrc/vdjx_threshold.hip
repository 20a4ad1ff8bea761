// vdjx_threshold.hip -- the lineage threshold: the valley between the two modes of the nearest-neighbour distances (gfx950 only, wave64).
//
//   vdjx_lineage_threshold   shazam's findThreshold(method = "density") in integers: the nearest distances of vdjx_lineage go into 10,001
//                            bins of 0.0001, the counts are smoothed with a Gaussian of every bandwidth k / 1000, k = 1 .. max_k, and the
//                            smallest bandwidth that leaves two modes gives the valley (the model: include/vdjx.h; in Python:
//                            tests/threshold_model.py)
//   vdjx_threshold_kernel    plain C, no GPU: the fixed-point Gaussian of one bandwidth
//
// Five dispatches whatever n is (and the clearing of the counters before them):
//   k_thr_hist      a thread per item: its bin (a clamped 64-bit quotient, by compare and subtract), counted with ds_add into the workgroup's
//                   10,001 LDS counters; a workgroup then adds its non-zero counters to the global ones, one integer atomic each
//   k_scan_one      (vdjx_scan.h) numbers the non-zero bins
//   k_thr_compact   the ascending (v, c) list of the non-zero bins
//   k_thr_density   grid (tiles of THR_TILE grid points, k): w_k[0 .. len_k) in LDS (at most 40 KB), a thread per g.  Two binary searches
//                   give the bins within len_k - 1 of the tile; they go through LDS in chunks and every one is read back as one 8-byte
//                   broadcast, w_k[|g - v|] at consecutive addresses in consecutive lanes, one 32 x 32 + 64 multiply-add a term; a lane
//                   further than the table's length from the bin adds 0.  Small k: short tables, short windows
//   k_thr_peaks     a workgroup per k: the row's maximum, then every point that begins a run higher than the point before it walks its
//                   run (a run of zeros begins no such run and is never walked) and knows whether it is a peak; the counts and the two
//                   first counted peaks (two LDS atomicMin passes over the starts) make the row's record
// The host picks k* from the max_k records and brings down that one row (80 KB), the histogram and the records; the valley is a walk over
// that row between the two peaks.  The max_k x (G + 1) matrix (16 MB) stays on the device.  No floating point on the device, integer atomics
// only (sums and minima: the order they land in changes nothing).  Every buffer comes from the context's workspace.
#include "vdjx_common.h"
#include "vdjx_scan.h"

#include <math.h>
#include <string.h>

#include <mutex>

#define THR_G VDJX_THRESHOLD_GRID        // the grid is g = 0 .. THR_G
#define THR_N (THR_G + 1u)
#define THR_FIX (1u << 30)
#define THR_TILE VDJX_THRESHOLD_TILE     // grid points per workgroup of k_thr_density
#define THR_CHUNK 256u                   // bins per LDS chunk there
#define THR_HIST_ITEMS 16384u            // items per workgroup of k_thr_hist
#define THR_NONE 0xFFFFFFFFu

struct ThrRow { u32 off, len; };                                               // where w_k's leading entries lie in the uploaded tables
struct ThrRec { u32 peaks_all, peaks, first[2], last[2]; u64 ymax, y[2]; };   // what k_thr_peaks leaves of a row
static_assert(sizeof(ThrRec) == 48, "downloaded as it is");

struct thr_nonzero {
	__device__ u32 operator()(u32 x) const { return x ? 1u : 0u; }
};

// min(G, num / den) for den > 0 and den (G + 1) < 2^63: the quotient has 14 bits once it is known to be below G + 1, so fourteen
// compare-and-subtract steps give it (the compiler's 64-bit division goes through a float reciprocal: exact, but floating point)
__device__ inline u32 thr_div_clamped(u64 num, u64 den) {
	if (num >= den * (u64) THR_N) return THR_G;
	u32 q = 0;
#pragma unroll
	for (int b = 13; b >= 0; b--) {
		const u64 s = den << b;
		if (s <= num) { num -= s; q |= 1u << b; }
	}
	return q;
}

// bin = min(G, (2 G nearest + unit L) / (2 unit L)): nearest < 2^31, unit <= 2^20 and L <= 255 keep both sides below 2^47
__global__ __launch_bounds__(1024) void k_thr_hist(const int32_t* __restrict__ nearest, const u32* __restrict__ length, u32 n, u32 unit, u32* __restrict__ hist) {
	__shared__ u32 cnt[THR_N];
	for (u32 i = threadIdx.x; i < THR_N; i += 1024u) cnt[i] = 0;
	__syncthreads();
	const u32 b0 = blockIdx.x * THR_HIST_ITEMS, b1 = min(n, b0 + THR_HIST_ITEMS);
	for (u32 i = b0 + threadIdx.x; i < b1; i += 1024u) {
		const int32_t d = nearest[i];
		if (d < 0) continue;
		const u64 ul = (u64) unit * length[i];
		atomicAdd(&cnt[thr_div_clamped(2ull * THR_G * (u64) d + ul, 2ull * ul)], 1u);
	}
	__syncthreads();
	for (u32 i = threadIdx.x; i < THR_N; i += 1024u) {
		const u32 x = cnt[i];
		if (x) atomicAdd(hist + i, x);
	}
}

// pos: the exclusive prefix of the non-zero flags (THR_N + 1 entries)
__global__ __launch_bounds__(256) void k_thr_compact(const u32* __restrict__ hist, const u32* __restrict__ pos, uint2* __restrict__ bins) {
	const u32 v = blockIdx.x * 256u + threadIdx.x;
	if (v >= THR_N) return;
	const u32 x = hist[v];
	if (x) bins[pos[v]] = make_uint2(v, x);
}

// Y_k[g] = the sum over the bins of c[v] w_k[|g - v|].  blockIdx.x: the tile of g, blockIdx.y: k - 1; *nbins: the length of the list
__global__ __launch_bounds__(THR_TILE) void k_thr_density(const uint2* __restrict__ bins, const u32* __restrict__ nbins, const ThrRow* __restrict__ rows,
                                                          const u32* __restrict__ tables, u64* __restrict__ Y) {
	__shared__ u32 w[THR_N];
	__shared__ uint2 chunk[THR_CHUNK];
	const ThrRow row = rows[blockIdx.y];
	const u32 len = row.len;                                 // 1 .. THR_N
	for (u32 i = threadIdx.x; i < len; i += THR_TILE) w[i] = tables[row.off + i];
	const u32 g0 = blockIdx.x * THR_TILE, g1 = min(g0 + THR_TILE - 1u, THR_G), g = g0 + threadIdx.x, nb = *nbins;
	// the bins with v + len - 1 >= g0 and v - (len - 1) <= g1
	const u32 vlo = g0 >= len - 1u ? g0 - (len - 1u) : 0u, vhi = g1 + (len - 1u);
	u32 lo = 0, hi = nb;
	while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (bins[mid].x < vlo) lo = mid + 1u; else hi = mid; }
	const u32 first = lo;
	hi = nb;
	while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (bins[mid].x <= vhi) lo = mid + 1u; else hi = mid; }
	const u32 end = lo;
	u64 acc = 0;
	for (u32 base = first; base < end; base += THR_CHUNK) {
		const u32 nc = min(THR_CHUNK, end - base);
		__syncthreads();                                     // (the table is in place; the chunk before has been read)
		for (u32 i = threadIdx.x; i < nc; i += THR_TILE) chunk[i] = bins[base + i];
		__syncthreads();
		for (u32 j = 0; j < nc; j++) {
			const uint2 b = chunk[j];                        // (every lane the same address: one broadcast read of 8 bytes)
			const u32 d = g >= b.x ? g - b.x : b.x - g;
			const u32 x = d < len ? w[d] : 0u;
			acc += (u64) b.y * x;
		}
	}
	if (g <= THR_G) Y[(size_t) blockIdx.y * THR_N + g] = acc;
}

// the run that begins at g (Y[g - 1] < Y[g] or g == 0, and Y[g] > 0): its last point, and whether what follows is lower
__device__ inline bool thr_peak_at(const u64* __restrict__ y, u32 g, u32& last) {
	const u64 v = y[g];
	u32 e = g;
	while (e < THR_G && y[e + 1u] == v) e++;
	last = e;
	return e == THR_G || y[e + 1u] < v;
}

// one workgroup per row
__global__ __launch_bounds__(256) void k_thr_peaks(const u64* __restrict__ Y, u32 shift, ThrRec* __restrict__ recs) {
	__shared__ u64 part[4];
	__shared__ u32 s_all, s_cnt, s_first, s_second;
	const u64* y = Y + (size_t) blockIdx.x * THR_N;
	const u32 t = threadIdx.x;
	u64 mx = 0;
	for (u32 g = t; g < THR_N; g += 256u) mx = max(mx, y[g]);
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) mx = max(mx, (u64) __shfl_xor((long long) mx, s, 64));
	if ((t & 63u) == 0) part[t >> 6] = mx;
	if (t == 0) { s_all = 0; s_cnt = 0; s_first = THR_NONE; s_second = THR_NONE; }
	__syncthreads();
	const u64 ymax = max(max(part[0], part[1]), max(part[2], part[3]));
	u32 all = 0, cnt = 0, mine = THR_NONE;                  // this thread's peaks, and the lowest start of its counted ones
	for (u32 g = t; g < THR_N; g += 256u) {
		const u64 v = y[g];
		if (v == 0 || (g > 0 && y[g - 1u] >= v)) continue;
		u32 last;
		if (!thr_peak_at(y, g, last)) continue;
		all++;
		if ((v << shift) >= ymax) { cnt++; mine = min(mine, g); }
	}
	if (all) atomicAdd(&s_all, all);
	if (cnt) { atomicAdd(&s_cnt, cnt); atomicMin(&s_first, mine); }
	__syncthreads();
	const u32 p1 = s_first;
	if (s_cnt >= 2u) {                                       // the second: the lowest counted start above the first
		u32 next = THR_NONE;
		for (u32 g = t; g < THR_N; g += 256u) {
			const u64 v = y[g];
			if (g <= p1 || v == 0 || y[g - 1u] >= v || (v << shift) < ymax) continue;
			u32 last;
			if (thr_peak_at(y, g, last)) { next = g; break; }   // (a thread's points ascend)
		}
		if (next != THR_NONE) atomicMin(&s_second, next);
	}
	__syncthreads();
	if (t == 0) {
		ThrRec r;
		r.peaks_all = s_all;
		r.peaks = s_cnt;
		r.ymax = ymax;
		const u32 p[2] = {p1, s_second};
		for (int i = 0; i < 2; i++) {
			r.first[i] = r.last[i] = 0;
			r.y[i] = 0;
			if (p[i] == THR_NONE) continue;
			r.first[i] = p[i];
			thr_peak_at(y, p[i], r.last[i]);
			r.y[i] = y[p[i]];
		}
		recs[blockIdx.x] = r;
	}
}

// ---- the host's tables: built once per process --------------------------------------------------------------------------------------
// w[d] = floor(FIX exp(-(double)(d d) / (double)(200 k k)) + 0.5) up to the first 0, zeros after it (the table does not increase).  One
// float64 operation per statement: the Python model (tests/threshold_model.py), which calls the same libm, gives the same integers
static u32 thr_kernel_fill(int k, uint32_t* w) {
	const double den = (double) (200 * k * k);
	u32 len = 0;
	while (len < THR_N) {
		const double num = -(double) (len * len);
		const double e = exp(num / den);
		const double s = (double) THR_FIX * e;
		const u32 x = (u32) floor(s + 0.5);
		if (x == 0) break;
		w[len++] = x;
	}
	for (u32 d = len; d < THR_N; d++) w[d] = 0;
	return len;
}

extern "C" int vdjx_threshold_kernel(int k, uint32_t* w, uint32_t* len) {
	if (len) *len = 0;
	if (k < 1 || k > VDJX_THRESHOLD_MAX_K) { vdjx_set_error("vdjx_threshold_kernel: k %d (1 .. %d)", k, VDJX_THRESHOLD_MAX_K); return VDJX_EINVAL; }
	if (!w) { vdjx_set_error("vdjx_threshold_kernel: NULL table"); return VDJX_EINVAL; }
	const u32 n = thr_kernel_fill(k, w);
	if (len) *len = n;
	return VDJX_OK;
}

struct ThrTables {
	std::vector<u32> w;                                    // the leading non-zero entries of every k, one after another (about 5 MB)
	ThrRow row[VDJX_THRESHOLD_MAX_K];
	u64 build_us = 0;
};
static const ThrTables& thr_tables() {
	static ThrTables T;
	static std::once_flag once;
	std::call_once(once, [] {
		const auto t0 = std::chrono::steady_clock::now();
		std::vector<u32> one(THR_N);
		for (int k = 1; k <= VDJX_THRESHOLD_MAX_K; k++) {
			const u32 len = thr_kernel_fill(k, one.data());
			T.row[k - 1] = {(u32) T.w.size(), len};
			T.w.insert(T.w.end(), one.begin(), one.begin() + len);
		}
		T.build_us = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	});
	return T;
}

extern "C" int vdjx_lineage_threshold(vdjx_ctx* c, const int32_t* nearest, const uint32_t* length, size_t n, uint32_t unit, const vdjx_threshold_params* prm,
                                      uint32_t* out_hist, uint64_t* out_density, uint32_t* out_peaks, vdjx_threshold_info* info) {
	const char* fn = "vdjx_lineage_threshold";
	if (!c || !prm || !info) { vdjx_set_error("%s: NULL argument", fn); return VDJX_EINVAL; }
	memset(info, 0, sizeof *info);
	if (prm->max_k < 1 || prm->max_k > VDJX_THRESHOLD_MAX_K) { vdjx_set_error("%s: max_k %d (1 .. %d)", fn, prm->max_k, VDJX_THRESHOLD_MAX_K); return VDJX_EINVAL; }
	if (prm->peak_shift < 0 || prm->peak_shift > 13) { vdjx_set_error("%s: peak_shift %d (0 .. 13)", fn, prm->peak_shift); return VDJX_EINVAL; }
	if (prm->valley_den < 1 || prm->valley_den > 1000000 || prm->valley_num < 0 || prm->valley_num > prm->valley_den) {
		vdjx_set_error("%s: valley guard %d/%d (den 1 .. 10^6, num 0 .. den)", fn, prm->valley_num, prm->valley_den);
		return VDJX_EINVAL;
	}
	if (prm->min_values < 1) { vdjx_set_error("%s: min_values %d (at least 1)", fn, prm->min_values); return VDJX_EINVAL; }
	if (unit == 0 || unit > (1u << 20)) { vdjx_set_error("%s: unit %u (1 .. 2^20)", fn, unit); return VDJX_EINVAL; }
	if (n >= (1ull << 20)) { vdjx_set_error("%s: %zu items (at most 2^20 - 1 per call)", fn, n); return VDJX_EINVAL; }
	if (n && (!nearest || !length)) { vdjx_set_error("%s: NULL argument", fn); return VDJX_EINVAL; }
	const auto t0 = std::chrono::steady_clock::now();
	u32 values = 0;
	for (size_t i = 0; i < n; i++) {
		if (nearest[i] < -1) { vdjx_set_error("%s: item %zu has nearest %d (-1: none)", fn, i, nearest[i]); return VDJX_EINVAL; }
		if (nearest[i] < 0) continue;
		if (length[i] == 0 || length[i] > 255u) { vdjx_set_error("%s: item %zu has length %u (1 .. 255)", fn, i, length[i]); return VDJX_EINVAL; }
		values++;
	}
	const u32 K = (u32) prm->max_k;
	vdjx_threshold_info inf;
	memset(&inf, 0, sizeof inf);
	inf.values = values;
	inf.status = VDJX_THRESHOLD_FEW;
	if (out_density) memset(out_density, 0, THR_N * sizeof(uint64_t));
	if (out_peaks) memset(out_peaks, 0, (size_t) K * 2 * sizeof(uint32_t));
	c->stats["threshold_macs"] = 0;
	if (values == 0) {                                       // nothing to count: no dispatch
		if (out_hist) memset(out_hist, 0, THR_N * sizeof(uint32_t));
		*info = inf;
		c->stats["threshold_us"] = 0;
		return VDJX_OK;
	}
	const bool dense = values >= (u32) prm->min_values;     // status 1: the histogram alone
	const ThrTables& T = thr_tables();
	const size_t wn = (size_t) T.row[K - 1].off + T.row[K - 1].len;

	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	vdjx_work wk(c);
	int32_t* d_near;
	u32 *d_len, *d_hist, *d_pos, *d_tab = nullptr;
	uint2* d_bins;
	ThrRow* d_rows = nullptr;
	u64* d_Y = nullptr;
	ThrRec* d_recs = nullptr;
	HIP_TRY(wk.alloc(&d_near, n));
	HIP_TRY(wk.alloc(&d_len, n));
	HIP_TRY(wk.alloc(&d_hist, THR_N));
	HIP_TRY(wk.alloc(&d_pos, THR_N + 1u));
	HIP_TRY(wk.alloc(&d_bins, THR_N));
	if (dense) {
		HIP_TRY(wk.alloc(&d_tab, wn));
		HIP_TRY(wk.alloc(&d_rows, K));
		HIP_TRY(wk.alloc(&d_Y, (size_t) K * THR_N));
		HIP_TRY(wk.alloc(&d_recs, K));
	}
	HIP_TRY(hipMemcpyAsync(d_near, nearest, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_len, length, n * sizeof(u32), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_hist, 0, THR_N * sizeof(u32), st));
	if (dense) {
		HIP_TRY(hipMemcpyAsync(d_tab, T.w.data(), wn * sizeof(u32), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_rows, T.row, K * sizeof(ThrRow), hipMemcpyHostToDevice, st));
	}
	{
		vdjx_prof_scope ps(c, "k_thr_hist");
		hipLaunchKernelGGL(k_thr_hist, dim3((u32) ((n + THR_HIST_ITEMS - 1u) / THR_HIST_ITEMS)), dim3(1024), 0, st, (const int32_t*) d_near, (const u32*) d_len, (u32) n,
		                   unit, d_hist);
	}
	if (dense) {
		{
			vdjx_prof_scope ps(c, "k_thr_number");
			vdjx_scan_one(st, (const u32*) d_hist, THR_N, d_pos, thr_nonzero());
		}
		{
			vdjx_prof_scope ps(c, "k_thr_compact");
			hipLaunchKernelGGL(k_thr_compact, dim3((THR_N + 255u) / 256u), dim3(256), 0, st, (const u32*) d_hist, (const u32*) d_pos, d_bins);
		}
		{
			vdjx_prof_scope ps(c, "k_thr_density");
			hipLaunchKernelGGL(k_thr_density, dim3((THR_N + THR_TILE - 1u) / THR_TILE, K), dim3(THR_TILE), 0, st, (const uint2*) d_bins, (const u32*) (d_pos + THR_N),
			                   (const ThrRow*) d_rows, (const u32*) d_tab, d_Y);
		}
		{
			vdjx_prof_scope ps(c, "k_thr_peaks");
			hipLaunchKernelGGL(k_thr_peaks, dim3(K), dim3(256), 0, st, (const u64*) d_Y, (u32) prm->peak_shift, d_recs);
		}
	}
	std::vector<u32> hist(THR_N);
	std::vector<ThrRec> recs(dense ? K : 0u);
	HIP_TRY(hipMemcpyAsync(hist.data(), d_hist, THR_N * sizeof(u32), hipMemcpyDeviceToHost, st));
	if (dense) HIP_TRY(hipMemcpyAsync(recs.data(), d_recs, K * sizeof(ThrRec), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	u64 macs = 0;
	for (u32 v = 0; v < THR_N; v++) {
		if (!hist[v]) continue;
		inf.distinct++;
		if (dense)                                           // the terms with a weight: the g within len_k - 1 of the bin, every k
			for (u32 k = 0; k < K; k++) macs += std::min(THR_G, v + T.row[k].len - 1u) - (v >= T.row[k].len - 1u ? v - (T.row[k].len - 1u) : 0u) + 1u;
	}
	if (out_hist) memcpy(out_hist, hist.data(), THR_N * sizeof(u32));
	if (dense) {
		u32 ks = 0;                                          // k*: the smallest k with at most two counted peaks
		while (ks < K && recs[ks].peaks > 2u) ks++;
		const bool none = ks == K;
		if (none) ks = K - 1u;
		std::vector<u64> y(THR_N);
		HIP_TRY(hipMemcpyAsync(y.data(), d_Y + (size_t) ks * THR_N, THR_N * sizeof(u64), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		const ThrRec& r = recs[ks];
		inf.k = ks + 1u;
		inf.peaks_all = r.peaks_all;
		inf.peaks = r.peaks;
		inf.ymax = r.ymax;
		inf.p1_first = r.first[0]; inf.p1_last = r.last[0]; inf.y1 = r.y[0];
		if (r.peaks >= 2u) { inf.p2_first = r.first[1]; inf.p2_last = r.last[1]; inf.y2 = r.y[1]; }
		if (none) inf.status = VDJX_THRESHOLD_NO_SCALE;
		else if (r.peaks < 2u) inf.status = VDJX_THRESHOLD_ONE_MODE;
		else {
			u64 m = ~0ull;
			for (u32 g = r.last[0] + 1u; g < r.first[1]; g++) {
				if (y[g] < m) { m = y[g]; inf.t_first = g; }
				if (y[g] == m) inf.t_last = g;
			}
			inf.m = m;
			const bool deep = (u64) prm->valley_den * m <= (u64) prm->valley_num * std::min(r.y[0], r.y[1]);      // (den <= 10^6 < 2^20, Y < 2^50)
			inf.status = deep ? VDJX_THRESHOLD_FOUND : VDJX_THRESHOLD_SHALLOW;
			if (deep) inf.threshold = (inf.t_first + inf.t_last) / 2u;
		}
		if (out_density) memcpy(out_density, y.data(), THR_N * sizeof(u64));
		if (out_peaks)
			for (u32 k = 0; k < K; k++) { out_peaks[2u * k] = recs[k].peaks_all; out_peaks[2u * k + 1u] = recs[k].peaks; }
	}
	vdjx_prof_collect(c, false);
	*info = inf;
	c->stats["threshold_macs"] = macs;
	c->stats["threshold_table_us"] = T.build_us;
	c->stats["threshold_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}
