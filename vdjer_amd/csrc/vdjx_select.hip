// vdjx_select.hip -- selection strength of the V segment's mutations, BASELINe's focused test (gfx950 only, wave64).
//
//   vdjx_selection   observed R / S counts per region, the expected R / S weights of the germline's codons under a 5-mer targeting model,
//                    and the posterior of the selection strength sigma per contig, per group and for all contigs (the model:
//                    include/vdjx.h; in Python: tests/selection_model.py)
//
// The hits are the caller's, so the host checks every one of them before anything reaches the device with the check vdjx_mutations uses
// (vh_check of vdjx_vhit.h): every index k_sel_counts forms lies inside the contig and the record.  The V segment table and the codon
// resolver are that header's too, so the two calls classify the same codons; what is here is what a resolved codon counts as.
//   k_sel_counts   one dispatch; a wave per contig, SEL_WAVES waves per workgroup, no barrier between the waves.  The V section of
//                  k_mutations' segment table (vh_hit_segments: 64 slots) in LDS, a lane per germline codon (vh_codon).  Per base of a
//                  classifiable codon: the region of its germline position, the observed class, and -- the germline codon not being a
//                  stop -- the three other bases through the amino-acid table, weighted by the 5-mer around the base in the RECORD (germline.d_cols; the record's bounds are
//                  checked, its neighbours in the set are never read as context).  The 1024 x 4 weights stay in global memory: a position
//                  reads the 16 bytes of its 5-mer with one load, a contig of 100 codons reads 4.8 KB of a 16 KB table that every wave
//                  shares, so it lives in L2 and the vector cache; staging it in LDS would cost every workgroup of four contigs the whole
//                  16 KB and a barrier.  int32 and uint64 wave reductions by shuffles; lane 0 writes the 64-byte row as four 16-byte
//                  stores.  No floating point, no atomics.
//   k_sel_loglik   rows with more than `chunk` members: a workgroup per (row, region, chunk of members) and tile of 256 grid points; a
//                  thread sums its grid point's terms over the chunk's members in order and writes partial[chunk][t].
//   k_sel_finish   a workgroup per (row, region): l[T] in LDS (32 KB), from its members directly or from the row's partials in chunk
//                  order, plus the prior; the block maximum, f = exp(l - max), a block scan for the CDF (a thread owns 16 consecutive grid
//                  points), the two quantile indices, sigma and p_positive; one 72-byte stat and, where asked, the density.
// No float atomics; every sum runs in a fixed order, so two calls with the same VDJX_SEL_CHUNK give the same bits.
#include "vdjx_vhit.h"
#include "vdjx_selpost.h"

#define SEL_WAVES 4

struct SelContig {
	u32 run_off;                         // V's runs in the pool
	u32 v_at;                            // the column of the hit's base germ_start in the set's columns
	u32 rec_at;                          // the column of the record's base 1
	u32 rec_len;
	u32 nruns;
	u32 flags;
	int v_seq0;                          // seq_start - 1
	int v_germ0;                         // germ_start - 1
	int limit;
	int cdr[4];                          // 1-based, inclusive; 0, 0: no such interval (all four 0 without a region map)
	int pad[3];
};
struct SelRow {                          // a row in a region
	u32 start, count;                    // its members in the region's member array
	u32 sequences;
	u32 part;                            // its first chunk of partials; SEL_DIRECT: summed from the members
	u32 nparts, pdf;                     // pdf: the density's row + 1, 0: none
	u64 x, n, exp_r, exp_s;
};
struct SelItem { u32 start, count, part, region; };    // a chunk of a large row's members
#define SEL_DIRECT 0xFFFFFFFFu
static_assert(sizeof(SelContig) == 64 && sizeof(SelRow) == 56,
              "uploaded / returned as they are");

__global__ __launch_bounds__(64 * SEL_WAVES) void k_sel_counts(const char* __restrict__ contigs, u32 n, u32 len, const SelContig* __restrict__ sc,
                                                              const u32* __restrict__ runs, const uint8_t* __restrict__ gcols,
                                                              const uint4* __restrict__ weight, int4* __restrict__ out) {
	__shared__ int4 seg_all[SEL_WAVES][65];
	__shared__ char aa_all[SEL_WAVES][64];
	const u32 w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const u32 c = blockIdx.x * SEL_WAVES + w;
	if (c >= n) return;                  // (a whole wave; nothing below waits for the others)
	int4* seg = seg_all[w];
	char* aa = aa_all[w];
	aa[lane] = vh_aa[lane];
	const SelContig q = sc[c];
	const char* ct = contigs + (size_t) c * len;
	// the V segment table, as k_mutations lays its V section: the hit starts at column 0, nothing is dropped
	int tc, tb, vgerm;
	seg[lane] = vh_hit_segments(runs, q.run_off, (int) q.nruns, lane, 0, q.v_seq0, (int) q.v_at, 0, 0, tc, tb, vgerm);
	vdjx_wave_lds_fence();               // the table and the amino acids are read by other lanes of the wave

	int obs_r[2] = {0, 0}, obs_s[2] = {0, 0}, ncod[2] = {0, 0};
	u64 exp_r[2] = {0, 0}, exp_s[2] = {0, 0};
	int c_lo, c_hi;
	vh_codon_range(q.v_germ0, vgerm, c_lo, c_hi);
	const int rlen = (int) q.rec_len;
	for (int cd = c_lo + (int) lane; cd < c_hi; cd += 64) {
		int cb[3], gb[3];
		if (!vh_codon(seg, ct, gcols, q.v_at, q.v_germ0, q.limit, cd, cb, gb)) continue;
		const int gc = 16 * gb[0] + 4 * gb[1] + gb[2];
		const char ga_ = aa[gc];
#pragma unroll
		for (int b = 0; b < 3; b++) {
			const int p = 3 * cd + b;            // the base's 0-based position in the record
			const int p1 = p + 1;
			const int reg = (p1 >= q.cdr[0] && p1 <= q.cdr[1]) || (p1 >= q.cdr[2] && p1 <= q.cdr[3]) ? 1 : 0;
			if (b == 0) ncod[reg]++;             // a codon belongs to the region of its first base
			if (cb[b] != gb[b]) {
				const char ma = vh_subst_aa(aa, gc, b, cb[b]);
				if (ga_ != '*' && ma != '*') {
					if (ga_ == ma) obs_s[reg]++; else obs_r[reg]++;
				}
			}
			if (ga_ == '*') continue;
			u32 wt[4] = {1u, 1u, 1u, 1u};
			if (weight) {
				if (p < 2 || p + 2 >= rlen) continue;
				const uint8_t* g5 = gcols + q.rec_at + (u32) (p - 2);
				const int g0 = g5[0], g1 = g5[1], g3 = g5[3], g4 = g5[4];
				if (g0 > 3 || g1 > 3 || g3 > 3 || g4 > 3) continue;      // (the centre is the codon's base: ACGT)
				const uint4 wv = weight[256 * g0 + 64 * g1 + 16 * gb[b] + 4 * g3 + g4];
				wt[0] = wv.x; wt[1] = wv.y; wt[2] = wv.z; wt[3] = wv.w;
			}
#pragma unroll
			for (int alt = 0; alt < 4; alt++) {
				if (alt == gb[b]) continue;
				const char ma = vh_subst_aa(aa, gc, b, alt);
				if (ma == '*') continue;
				if (ma == ga_) exp_s[reg] += wt[alt]; else exp_r[reg] += wt[alt];
			}
		}
	}
#pragma unroll
	for (int k = 0; k < 2; k++) {
		obs_r[k] = vdjx_wave_sum(obs_r[k]);
		obs_s[k] = vdjx_wave_sum(obs_s[k]);
		ncod[k] = vdjx_wave_sum(ncod[k]);
		exp_r[k] = vdjx_wave_sum64(exp_r[k]);
		exp_s[k] = vdjx_wave_sum64(exp_s[k]);
	}
	if (lane == 0) {
		int4* o = out + 4 * (size_t) c;
		o[0] = make_int4(obs_r[0], obs_r[1], obs_s[0], obs_s[1]);
		o[1] = make_int4(ncod[0], ncod[1], (int) q.flags, 0);
		o[2] = make_int4((int) (u32) exp_r[0], (int) (u32) (exp_r[0] >> 32), (int) (u32) exp_r[1], (int) (u32) (exp_r[1] >> 32));
		o[3] = make_int4((int) (u32) exp_s[0], (int) (u32) (exp_s[0] >> 32), (int) (u32) exp_s[1], (int) (u32) (exp_s[1] >> 32));
	}
}

// ---- the posterior -------------------------------------------------------------------------------------------------------------------------
// (sel_softplus, sel_sigma, sel_terms, the block reductions and the finish of a row: vdjx_selpost.h)
__global__ __launch_bounds__(256) void k_sel_loglik(const SelMember* __restrict__ members, size_t region_stride, const SelItem* __restrict__ items,
                                                    double* __restrict__ partial) {
	const SelItem it = items[blockIdx.y];
	const int t = (int) (blockIdx.x * 256 + threadIdx.x);
	if (t >= SEL_T) return;              // (the last tile: 161 of 256)
	partial[(size_t) it.part * SEL_T + (size_t) t] = sel_terms(members + (size_t) it.region * region_stride + it.start, it.count, sel_sigma(t));
}

__global__ __launch_bounds__(256) void k_sel_finish(const SelMember* __restrict__ members, size_t region_stride, const SelRow* __restrict__ rows,
                                                    u32 nrows, const double* __restrict__ partial, vdjx_sel_stat* __restrict__ out_stat,
                                                    double* __restrict__ out_pdf, u32 K) {
	__shared__ double ell[SEL_T];
	__shared__ double tot[256];
	__shared__ double red[4];
	__shared__ int qidx[2][4];
	const u32 row = blockIdx.x / K, region = blockIdx.x % K;
	const u32 tid = threadIdx.x;
	const SelRow rw = rows[(size_t) region * nrows + row];
	const SelMember* m = members + (size_t) region * region_stride + rw.start;
	// l[t], striped over the threads (t = tid + 256 j): uniform member reads, neighbouring partials
	double mx = -INFINITY;
	for (int t = (int) tid; t < SEL_T; t += 256) {
		const double sg = sel_sigma(t);
		double l = sg - 2.0 * sel_softplus(sg);
		if (rw.part == SEL_DIRECT) l += sel_terms(m, rw.count, sg);
		else {
			double acc = 0.0;
			for (u32 p = 0; p < rw.nparts; p++) acc += partial[(size_t) (rw.part + p) * SEL_T + (size_t) t];
			l += acc;
		}
		ell[t] = l;
		mx = fmax(mx, l);
	}
	mx = sel_block_max(mx, red);         // (its barriers publish ell)
	// f over 16 consecutive grid points per thread, then the row's finish
	const int t0 = (int) tid * SEL_PER;
	double f[SEL_PER];
#pragma unroll
	for (int j = 0; j < SEL_PER; j++) f[j] = t0 + j < SEL_T ? exp(ell[t0 + j] - mx) : 0.0;
	sel_finish_tail(f, ell, tot, red, qidx, rw.sequences, rw.x, rw.n, rw.exp_r, rw.exp_s, out_stat + (size_t) row * K + region,
	                out_pdf && rw.pdf ? out_pdf + ((size_t) (rw.pdf - 1) * K + region) * SEL_T : nullptr);
}

// ---- the host's side -------------------------------------------------------------------------------------------------------------------------
extern "C" int vdjx_selection(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_annot_hit* v, const int32_t* limit, const int32_t* cdr,
                              size_t n_records, const uint32_t* weight, const int32_t* group, uint32_t G, vdjx_sel_counts* out_counts,
                              vdjx_sel_stat* out_stat, double* out_pdf, vdjx_sel_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("vdjx_selection: NULL argument"); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!contigs || !v || !out_counts || !out_stat) { vdjx_set_error("vdjx_selection: NULL argument"); return VDJX_EINVAL; }
	int rc = vh_check_sizes("vdjx_selection", n, len);
	if (rc != VDJX_OK) return rc;
	if (G >= (1u << 20)) { vdjx_set_error("vdjx_selection: %u groups (at most 2^20 - 1)", G); return VDJX_EINVAL; }
	if (G && !group) { vdjx_set_error("vdjx_selection: %u groups and no group array", G); return VDJX_EINVAL; }
	if (out_pdf && (u64) G + 1 > 65536) { vdjx_set_error("vdjx_selection: densities of %u groups and the sample (at most 65536 rows)", G); return VDJX_EINVAL; }
	rc = vh_check_contigs("vdjx_selection", c, contigs, n, len);
	if (rc != VDJX_OK) return rc;
	const vdjx_recset& gs = c->germline;
	if (cdr) {
		if (n_records != gs.given) {
			vdjx_set_error("vdjx_selection: a region map of %zu records, %zu records were loaded", n_records, gs.given);
			return VDJX_EINVAL;
		}
		for (size_t s = 0; s < gs.rec[0].size(); s++) {
			const int32_t* iv = cdr + 4 * (size_t) gs.rec[0][s];
			if (iv[0] == -1) continue;
			for (int k = 0; k < 4; k += 2) {
				if (iv[k] == 0 && iv[k + 1] == 0) continue;
				if (iv[k] < 1 || iv[k] > iv[k + 1] || (int64_t) iv[k + 1] > (int64_t) gs.len[0][s]) {
					vdjx_set_error("vdjx_selection: record %u: the interval %d .. %d (1 <= start <= end <= %u, or 0 0)", gs.rec[0][s], iv[k], iv[k + 1], gs.len[0][s]);
					return VDJX_EINVAL;
				}
			}
		}
	}
	const u32 K = cdr ? 2 : 1;
	const long long chunk_ll = vdjx_env_num("VDJX_SEL_CHUNK", 1024, 1, 65536);
	const u32 chunk = (u32) chunk_ll;
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<SelContig> sc(n);
	std::vector<u32> runs;
	u64 truncated = 0, no_regions = 0;
	for (size_t i = 0; i < n; i++) {
		const int lim = limit ? limit[i] : len;
		if (lim < 0 || lim > len) { vdjx_set_error("vdjx_selection: contig %zu: limit %d (0 .. %d)", i, lim, len); return VDJX_EINVAL; }
		if (group && G && group[i] >= 0 && (u32) group[i] >= G) { vdjx_set_error("vdjx_selection: contig %zu: group %d of %u", i, group[i], G); return VDJX_EINVAL; }
		SelContig& q = sc[i];
		memset(&q, 0, sizeof q);
		q.limit = lim;
		q.run_off = (u32) runs.size();
		if (vh_called(v[i]) && !vh_usable(v[i])) { q.flags = 16; truncated++; continue; }
		if (!vh_usable(v[i])) continue;
		size_t slot = 0;
		rc = vh_check("vdjx_selection", "V", i, v[i], gs, 0, len, &slot);
		if (rc != VDJX_OK) return rc;
		if (cdr) {
			const int32_t* iv = cdr + 4 * (size_t) v[i].gene;
			if (iv[0] == -1) { q.flags = 32; no_regions++; continue; }
			for (int k = 0; k < 4; k++) q.cdr[k] = iv[k];
		}
		q.flags = 1;
		q.nruns = (u32) v[i].n_runs;
		runs.insert(runs.end(), v[i].runs, v[i].runs + q.nruns);
		q.rec_at = (u32) (gs.at[0][slot] + 1);
		q.rec_len = gs.len[0][slot];
		q.v_at = (u32) (gs.at[0][slot] + (u64) v[i].germ_start);
		q.v_seq0 = v[i].seq_start - 1;
		q.v_germ0 = v[i].germ_start - 1;
	}

	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	vdjx_work wk(c);
	char* d_ct;
	SelContig* d_sc;
	u32 *d_runs, *d_w = nullptr;
	int4* d_out;
	HIP_TRY(wk.alloc(&d_ct, n * (size_t) len));
	HIP_TRY(wk.alloc(&d_sc, n));
	HIP_TRY(wk.alloc(&d_runs, runs.size()));
	HIP_TRY(wk.alloc(&d_out, 4 * n));
	HIP_TRY(hipMemcpyAsync(d_ct, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_sc, sc.data(), n * sizeof(SelContig), hipMemcpyHostToDevice, st));
	if (!runs.empty()) HIP_TRY(hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(u32), hipMemcpyHostToDevice, st));
	if (weight) {
		HIP_TRY(wk.alloc(&d_w, 4096));
		HIP_TRY(hipMemcpyAsync(d_w, weight, 4096 * sizeof(u32), hipMemcpyHostToDevice, st));
	}
	{
		vdjx_prof_scope ps(c, "k_sel_counts");
		hipLaunchKernelGGL(k_sel_counts, dim3((u32) ((n + SEL_WAVES - 1) / SEL_WAVES)), dim3(64 * SEL_WAVES), 0, st, (const char*) d_ct, (u32) n, (u32) len,
		                   (const SelContig*) d_sc, (const u32*) d_runs, (const uint8_t*) c->germline.d_cols, (const uint4*) d_w, d_out);
	}
	HIP_TRY(hipMemcpyAsync(out_counts, d_out, n * sizeof(vdjx_sel_counts), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());

	// the members: per region the contigs in order, then the grouped contigs by group (contig order inside a group)
	std::vector<u32> gstart, gorder;
	sel_group_order(group, n, G, gstart, gorder);
	const size_t ng = gorder.size(), stride = n + ng, nrows = n + G + 1;
	std::vector<SelMember> mem(K * stride);
	std::vector<SelRow> rows(K * nrows);
	std::vector<SelItem> items;
	u32 nparts = 0, large_rows = 0;
	u64 used = 0;
	for (size_t i = 0; i < n; i++) used += (out_counts[i].flags & 1u) != 0;
	for (u32 k = 0; k < K; k++) {
		SelMember* m = mem.data() + k * stride;
		for (size_t i = 0; i < n; i++) m[i] = sel_member(out_counts[i], k, K);
		for (size_t a = 0; a < ng; a++) m[n + a] = m[gorder[a]];
		SelRow* rw = rows.data() + k * nrows;
		for (size_t r = 0; r < nrows; r++) {
			SelRow& R = rw[r];
			memset(&R, 0, sizeof R);
			if (r < n) { R.start = (u32) r; R.count = 1; }
			else if (r < n + G) { R.start = (u32) (n + gstart[r - n]); R.count = gstart[r - n + 1] - gstart[r - n]; R.pdf = out_pdf ? (u32) (r - n) + 1 : 0; }
			else { R.start = 0; R.count = (u32) n; R.pdf = out_pdf ? G + 1 : 0; }
			for (u32 a = 0; a < R.count; a++) {
				const SelMember& e = m[R.start + a];
				if (!e.n) continue;
				const size_t i = R.start + a < n ? R.start + a : gorder[R.start + a - n];
				u64 es = 0;
				for (u32 j = 0; j < K; j++) es += out_counts[i].exp_s[j];
				R.sequences++;
				R.x += e.x; R.n += e.n; R.exp_r += out_counts[i].exp_r[k]; R.exp_s += es;
			}
			R.part = SEL_DIRECT;
			if (R.count > chunk) {
				R.part = nparts;
				R.nparts = (R.count + chunk - 1) / chunk;
				for (u32 p = 0; p < R.nparts; p++) items.push_back({R.start + p * chunk, std::min(chunk, R.count - p * chunk), nparts + p, k});
				nparts += R.nparts;
				large_rows += k == 0;
			}
		}
	}
	SelMember* d_mem;
	SelRow* d_rows;
	SelItem* d_items;
	double *d_partial, *d_pdf = nullptr;
	vdjx_sel_stat* d_stat;
	HIP_TRY(wk.alloc(&d_mem, mem.size()));
	HIP_TRY(wk.alloc(&d_rows, rows.size()));
	HIP_TRY(wk.alloc(&d_items, items.size()));
	HIP_TRY(wk.alloc(&d_partial, (size_t) nparts * SEL_T));
	HIP_TRY(wk.alloc(&d_stat, nrows * K));
	if (out_pdf) HIP_TRY(wk.alloc(&d_pdf, (size_t) (G + 1) * K * SEL_T));
	HIP_TRY(hipMemcpyAsync(d_mem, mem.data(), mem.size() * sizeof(SelMember), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(SelRow), hipMemcpyHostToDevice, st));
	if (!items.empty()) {
		HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(SelItem), hipMemcpyHostToDevice, st));
		for (size_t a = 0; a < items.size(); a += 65535) {       // (a launch's second grid dimension holds 65,535)
			vdjx_prof_scope ps(c, "k_sel_loglik");
			hipLaunchKernelGGL(k_sel_loglik, dim3((SEL_T + 255) / 256, (u32) std::min<size_t>(65535, items.size() - a)), dim3(256), 0, st,
			                   (const SelMember*) d_mem, stride, (const SelItem*) d_items + a, d_partial);
		}
	}
	{
		vdjx_prof_scope ps(c, "k_sel_finish");
		hipLaunchKernelGGL(k_sel_finish, dim3((u32) (nrows * K)), dim3(256), 0, st, (const SelMember*) d_mem, stride, (const SelRow*) d_rows, (u32) nrows,
		                   (const double*) d_partial, d_stat, d_pdf, K);
	}
	HIP_TRY(hipMemcpyAsync(out_stat, d_stat, nrows * K * sizeof(vdjx_sel_stat), hipMemcpyDeviceToHost, st));
	if (out_pdf) HIP_TRY(hipMemcpyAsync(out_pdf, d_pdf, (size_t) (G + 1) * K * SEL_T * sizeof(double), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	vdjx_prof_collect(c, false);
	if (info) {
		info->contigs = n;
		info->used = used;
		info->no_regions = no_regions;
		info->truncated = truncated;
		info->groups = G;
		info->regions = K;
		info->chunks = nparts;
		info->large_rows = large_rows;
	}
	c->stats["selection_chunks"] = nparts;
	c->stats["selection_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}
