// vdjx_target.hip -- the sample's own 5-mer targeting model, shazam's createTargetingModel (gfx950 only, wave64).
//
//   vdjx_targeting_counts   per 5-mer and new base, how often the sample's V segments showed the change (observed) and how often the 5-mer was
//                           there to show it (opportunity), silent and replacement apart; a lineage's members over one record count once
//   vdjx_targeting_model    plain C, no GPU: the counts -> the S5F weights vdjx_selection takes (the model of both: include/vdjx.h; in Python:
//                           tests/targeting_model.py)
//
// The hits are the caller's, checked on the host exactly as vdjx_selection checks them (vh_check of vdjx_vhit.h); the V segment table and the
// codon resolver are that header's, so the three calls classify the same codons.  A UNIT is a (group, V record) pair; it owns a bitmap of 4 bits
// per record position (256 words: 1 KB), bit b of position p: "base b was seen at p" -- the germline base: the position was there to mutate;
// another base: that change was observed.  Counting the SET bits, not the contigs, is what makes a lineage's shared mutation one event and the
// result a function of the set alone: no order of contigs, members or batches can show.
//   k_tgt_mark    per batch of units; a wave per contig, TGT_WAVES waves per workgroup, no barrier.  k_sel_counts' walk: the V section of the
//                 segment table in LDS, a lane per germline codon (vh_codon).  A codon's three nibbles go out as one or two 32-bit atomicOr
//                 into the unit's words; a word that already holds them is skipped (a plain read first: members of a lineage mostly repeat
//                 each other).
//   k_tgt_count   per batch; a wave per unit, TGT_WAVES waves per workgroup striding over the batch's units, with one histogram of
//                 2 x 2 x 1024 x 3 u32 per workgroup in LDS (48 KB: the centre base has no counter).  A lane loads four of the unit's
//                 256 words at once; for a non-empty word (8 positions) it reads the 12 record bases around them once and adds with integer
//                 LDS atomics; at the end a workgroup adds its non-zero counters to the call's uint64 counters with 64-bit global atomics.
//                 A workgroup's u32 cannot overflow: a batch holds fewer than 2^20 units of at most 2,047 positions.
// No floating point on the device, integer atomics only: they commute, so two calls give the same bytes.
#include "vdjx_vhit.h"

#include <math.h>

#define TGT_WAVES 4
#define TGT_WORDS 256                    // a unit's bitmap: 8 positions of 4 bits per word, positions 0 .. 2047
#define TGT_BINS (2 * 2 * 1024 * 4)      // [kind][class][5-mer][new base]
#define TGT_HCLASS (1024 * 3)             // k_tgt_count's histogram: [kind][class][5-mer][new base but the centre], 48 KB
#define TGT_HBINS (2 * 2 * TGT_HCLASS)
#define TGT_COUNT_WGS 768                // k_tgt_count: three workgroups of 48 KB fit each of the 256 CUs

struct TgtContig {                       // a used contig, in unit order
	u32 run_off;                         // V's runs in the pool
	u32 v_at;                            // the column of the hit's base germ_start in the set's columns
	u32 rec_at;                          // the column of the record's base 1
	u32 rec_len;
	u32 nruns;
	u32 unit;
	u32 contig;                          // its index in the caller's block
	int v_seq0;                          // seq_start - 1
	int v_germ0;                         // germ_start - 1
	int limit;
	int pad[2];
};
struct TgtUnit { u32 rec_at, rec_len; };
static_assert(sizeof(TgtContig) == 48 && sizeof(TgtUnit) == 8 && sizeof(vdjx_tgt_info) == 80, "uploaded / returned as they are");
static_assert(TGT_HBINS * sizeof(u32) + 64 <= 65536, "k_tgt_count's histogram and the genetic code: within the LDS a kernel may declare");

__global__ __launch_bounds__(64 * TGT_WAVES) void k_tgt_mark(const char* __restrict__ contigs, u32 count, u32 len, const TgtContig* __restrict__ tc,
                                                            const u32* __restrict__ runs, const uint8_t* __restrict__ gcols, u32 unit0,
                                                            u32* __restrict__ bitmaps) {
	__shared__ int4 seg_all[TGT_WAVES][65];
	__shared__ char aa_all[TGT_WAVES][64];
	const u32 w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const u32 e = blockIdx.x * TGT_WAVES + w;
	if (e >= count) return;              // (a whole wave; nothing below waits for the others)
	int4* seg = seg_all[w];
	char* aa = aa_all[w];
	aa[lane] = vh_aa[lane];
	const TgtContig q = tc[e];
	const char* ct = contigs + (size_t) q.contig * len;
	u32* bm = bitmaps + (size_t) (q.unit - unit0) * TGT_WORDS;
	int tcols, tb, vgerm;
	seg[lane] = vh_hit_segments(runs, q.run_off, (int) q.nruns, lane, 0, q.v_seq0, (int) q.v_at, 0, 0, tcols, tb, vgerm);
	vdjx_wave_lds_fence();               // the table and the amino acids are read by other lanes of the wave

	int c_lo, c_hi;
	vh_codon_range(q.v_germ0, vgerm, c_lo, c_hi);
	const int rlen = (int) q.rec_len;
	for (int cd = c_lo + (int) lane; cd < c_hi; cd += 64) {
		int cb[3], gb[3];
		if (!vh_codon(seg, ct, gcols, q.v_at, q.v_germ0, q.limit, cd, cb, gb)) continue;
		const int gc = 16 * gb[0] + 4 * gb[1] + gb[2];
		if (aa[gc] == '*') continue;
		u32 nib = 0;                         // the codon's three nibbles
#pragma unroll
		for (int b = 0; b < 3; b++) {
			const int p = 3 * cd + b;            // the base's 0-based position in the record
			if (p < 2 || p + 2 >= rlen) continue;
			const uint8_t* g5 = gcols + q.rec_at + (u32) (p - 2);
			if (g5[0] > 3 || g5[1] > 3 || g5[3] > 3 || g5[4] > 3) continue;      // (the centre is the codon's base: ACGT)
			u32 v = 1u << gb[b];
			if (cb[b] != gb[b] && vh_subst_aa(aa, gc, b, cb[b]) != '*') v |= 1u << cb[b];
			nib |= v << (4 * b);
		}
		if (!nib) continue;
		const u32 p0 = (u32) (3 * cd);       // p0 + 2 <= 2046: word 255 is the last one touched
		const u64 vv = (u64) nib << (4u * (p0 & 7u));
		const u32 lo = (u32) vv, hi = (u32) (vv >> 32), wd = p0 >> 3;
		if (lo && (__atomic_load_n(bm + wd, __ATOMIC_RELAXED) & lo) != lo) atomicOr(bm + wd, lo);
		if (hi && (__atomic_load_n(bm + wd + 1, __ATOMIC_RELAXED) & hi) != hi) atomicOr(bm + wd + 1, hi);
	}
}

__global__ __launch_bounds__(64 * TGT_WAVES) void k_tgt_count(const TgtUnit* __restrict__ units, u32 nunits, const u32* __restrict__ bitmaps,
                                                             const uint8_t* __restrict__ gcols, u64* __restrict__ out) {
	__shared__ u32 hist[TGT_HBINS];
	__shared__ char aa[64];
	const u32 tid = threadIdx.x, w = tid >> 6, lane = tid & 63u;
	for (u32 i = tid; i < TGT_HBINS; i += 64 * TGT_WAVES) hist[i] = 0;
	if (tid < 64) aa[tid] = vh_aa[tid];
	__syncthreads();
	int seen = 0;
	for (u32 u = blockIdx.x * TGT_WAVES + w; u < nunits; u += gridDim.x * TGT_WAVES) {
		const u32* bm = bitmaps + (size_t) u * TGT_WORDS;
		const u32 w0 = bm[lane], w1 = bm[lane + 64], w2 = bm[lane + 128], w3 = bm[lane + 192];      // (four loads in flight, not four round trips)
		const TgtUnit un = units[u];
#pragma unroll 1
		for (u32 k = 0; k < 4; k++) {
			const u32 word = k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : w3;
			if (!word) continue;
			const u32 wd = lane + 64 * k;
			// record positions 8 wd - 2 .. 8 wd + 9, 4 bits each (4: not ACGT or outside the record; never under a set bit or beside one)
			u64 bases = 0;
#pragma unroll
			for (int q = 0; q < 12; q++) {
				const int idx = 8 * (int) wd - 2 + q;
				const u32 g = idx >= 0 && idx < (int) un.rec_len ? gcols[un.rec_at + (u32) idx] : 4u;
				bases |= (u64) (g & 7u) << (4 * q);
			}
#pragma unroll
			for (int j = 0; j < 8; j++) {
				const u32 nib = (word >> (4 * j)) & 15u;
				if (!nib) continue;
				seen++;
				const u32 five = (u32) (bases >> (4 * j)) & 0xFFFFFu;        // p - 2 .. p + 2, the first in the low nibble
				const int g0 = five & 3, g1 = (five >> 4) & 3, gb = (five >> 8) & 3, g3 = (five >> 12) & 3, g4 = (five >> 16) & 3;
				const int m = 256 * g0 + 64 * g1 + 16 * gb + 4 * g3 + g4;
				const int b = (int) ((8u * wd + (u32) j) % 3u);              // the base's place in its codon, whose first base is nibble j + 2 - b
				const u32 cod = (u32) (bases >> (4 * (j + 2 - b))) & 0xFFFu;
				const int gc = 16 * (int) (cod & 3u) + 4 * (int) ((cod >> 4) & 3u) + (int) ((cod >> 8) & 3u);
				const char ga = aa[gc];
#pragma unroll
				for (int x = 0; x < 4; x++) {
					if (x == gb) continue;
					const char ma = vh_subst_aa(aa, gc, b, x);
					if (ma == '*') continue;
					const u32 at = (ma == ga ? 0u : TGT_HCLASS) + 3u * (u32) m + (u32) (x - (x > gb));      // (the centre base has no counter)
					atomicAdd(&hist[2 * TGT_HCLASS + at], 1u);
					if ((nib >> x) & 1u) atomicAdd(&hist[at], 1u);
				}
			}
		}
	}
	__syncthreads();
	for (u32 i = tid; i < TGT_HBINS; i += 64 * TGT_WAVES) {
		const u32 v = hist[i];
		if (!v) continue;
		const u32 kc = i / TGT_HCLASS, r = i % TGT_HCLASS, m = r / 3u, x3 = r % 3u, x = x3 + (x3 >= ((m >> 4) & 3u));
		atomicAdd((unsigned long long*) out + (size_t) kc * 4096 + 4 * m + x, (unsigned long long) v);
	}
	seen = vdjx_wave_sum(seen);
	if (lane == 0 && seen) atomicAdd((unsigned long long*) out + TGT_BINS, (unsigned long long) seen);
}

// ---- the host's side -------------------------------------------------------------------------------------------------------------------------
extern "C" int vdjx_targeting_counts(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_annot_hit* v, const int32_t* limit,
                                     const int32_t* group, uint64_t* out, vdjx_tgt_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("vdjx_targeting_counts: NULL argument"); return VDJX_EINVAL; }
	if (n == 0) {
		if (out) memset(out, 0, TGT_BINS * sizeof(uint64_t));
		return VDJX_OK;
	}
	if (!contigs || !v || !out) { vdjx_set_error("vdjx_targeting_counts: NULL argument"); return VDJX_EINVAL; }
	int rc = vh_check_sizes("vdjx_targeting_counts", n, len);
	if (rc != VDJX_OK) return rc;
	rc = vh_check_contigs("vdjx_targeting_counts", c, contigs, n, len);
	if (rc != VDJX_OK) return rc;
	const vdjx_recset& gs = c->germline;
	const u32 per_batch = (u32) vdjx_env_num("VDJX_TGT_UNITS", 1 << 18, 1, (1 << 20) - 1);
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<TgtContig> tc;
	std::vector<std::pair<u64, u32>> order;      // (the unit's key, the contig's place in tc)
	std::vector<u32> runs;
	tc.reserve(n);
	u64 truncated = 0;
	for (size_t i = 0; i < n; i++) {
		const int lim = limit ? limit[i] : len;
		if (lim < 0 || lim > len) { vdjx_set_error("vdjx_targeting_counts: contig %zu: limit %d (0 .. %d)", i, lim, len); return VDJX_EINVAL; }
		if (vh_called(v[i]) && !vh_usable(v[i])) { truncated++; continue; }
		if (!vh_usable(v[i])) continue;
		size_t slot = 0;
		rc = vh_check("vdjx_targeting_counts", "V", i, v[i], gs, 0, len, &slot);
		if (rc != VDJX_OK) return rc;
		TgtContig q;
		memset(&q, 0, sizeof q);
		q.limit = lim;
		q.run_off = (u32) runs.size();
		q.nruns = (u32) v[i].n_runs;
		runs.insert(runs.end(), v[i].runs, v[i].runs + q.nruns);
		q.rec_at = (u32) (gs.at[0][slot] + 1);
		q.rec_len = gs.len[0][slot];
		q.v_at = (u32) (gs.at[0][slot] + (u64) v[i].germ_start);
		q.contig = (u32) i;
		q.v_seq0 = v[i].seq_start - 1;
		q.v_germ0 = v[i].germ_start - 1;
		// a unit: (group, V record); a contig in no group is a unit of its own (n < 2^20 <= the slots' 2^31)
		const u64 key = group && group[i] >= 0 ? (u64) (u32) group[i] << 32 | (u64) slot : 1ull << 63 | (u64) i;
		order.push_back({key, (u32) tc.size()});
		tc.push_back(q);
	}
	// the contigs by unit, so that a batch of whole units is a range of them
	std::sort(order.begin(), order.end());
	const size_t used = tc.size();
	std::vector<TgtContig> sorted(used);
	std::vector<TgtUnit> units;
	std::vector<u32> first;                  // a unit's first contig in `sorted`; one more entry: used
	for (size_t a = 0; a < used; a++) {
		if (a == 0 || order[a].first != order[a - 1].first) {
			first.push_back((u32) a);
			units.push_back({tc[order[a].second].rec_at, tc[order[a].second].rec_len});
		}
		sorted[a] = tc[order[a].second];
		sorted[a].unit = (u32) units.size() - 1;
	}
	first.push_back((u32) used);
	const u32 nunits = (u32) units.size();
	const u32 batches = (nunits + per_batch - 1) / per_batch;

	std::vector<u64> tot(TGT_BINS + 1, 0);   // the counters, then the seen positions
	if (nunits) {
		HIP_TRY(hipSetDevice(c->device));
		hipStream_t st = c->stream;
		vdjx_work wk(c);
		char* d_ct;
		TgtContig* d_tc;
		TgtUnit* d_units;
		u32 *d_runs, *d_bm;
		u64* d_out;
		const u32 cap = std::min(nunits, per_batch);
		HIP_TRY(wk.alloc(&d_ct, n * (size_t) len));
		HIP_TRY(wk.alloc(&d_tc, used));
		HIP_TRY(wk.alloc(&d_units, (size_t) nunits));
		HIP_TRY(wk.alloc(&d_runs, runs.size()));
		HIP_TRY(wk.alloc(&d_bm, (size_t) cap * TGT_WORDS));
		HIP_TRY(wk.alloc(&d_out, (size_t) TGT_BINS + 1));
		HIP_TRY(hipMemcpyAsync(d_ct, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_tc, sorted.data(), used * sizeof(TgtContig), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_units, units.data(), (size_t) nunits * sizeof(TgtUnit), hipMemcpyHostToDevice, st));
		if (!runs.empty()) HIP_TRY(hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(u32), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemsetAsync(d_out, 0, ((size_t) TGT_BINS + 1) * sizeof(u64), st));
		for (u32 u0 = 0; u0 < nunits; u0 += per_batch) {
			const u32 nu = std::min(per_batch, nunits - u0);
			const u32 c0 = first[u0], nc = first[u0 + nu] - c0;
			HIP_TRY(hipMemsetAsync(d_bm, 0, (size_t) nu * TGT_WORDS * sizeof(u32), st));
			{
				vdjx_prof_scope ps(c, "k_tgt_mark");
				hipLaunchKernelGGL(k_tgt_mark, dim3((nc + TGT_WAVES - 1) / TGT_WAVES), dim3(64 * TGT_WAVES), 0, st, (const char*) d_ct, nc, (u32) len,
				                   (const TgtContig*) d_tc + c0, (const u32*) d_runs, (const uint8_t*) c->germline.d_cols, u0, d_bm);
			}
			{
				vdjx_prof_scope ps(c, "k_tgt_count");
				hipLaunchKernelGGL(k_tgt_count, dim3(std::min<u32>(TGT_COUNT_WGS, (nu + TGT_WAVES - 1) / TGT_WAVES)), dim3(64 * TGT_WAVES), 0, st,
				                   (const TgtUnit*) d_units + u0, nu, (const u32*) d_bm, (const uint8_t*) c->germline.d_cols, d_out);
			}
		}
		HIP_TRY(hipMemcpyAsync(tot.data(), d_out, tot.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(hipGetLastError());
		vdjx_prof_collect(c, false);
	}
	memcpy(out, tot.data(), TGT_BINS * sizeof(uint64_t));
	if (info) {
		info->contigs = n;
		info->used = used;
		info->truncated = truncated;
		info->units = nunits;
		info->positions = tot[TGT_BINS];
		for (u32 i = 0; i < 4096; i++) {
			info->obs_s += tot[i];
			info->obs_r += tot[4096 + i];
			info->opp_s += tot[8192 + i];
			info->opp_r += tot[12288 + i];
		}
		info->batches = batches;
	}
	c->stats["targeting_units"] = nunits;
	c->stats["targeting_batches"] = batches;
	c->stats["targeting_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}

// plain C, no GPU: the S5F finish.  One float64 operation per statement: no product feeds a sum, so nothing can be contracted and the numpy
// model (tests/targeting_model.py), which does the same operations in the same order, gives the same integers
extern "C" int vdjx_targeting_model(const uint64_t* counts, int cls, uint64_t min_sub, uint64_t min_mut, uint32_t* out_weight, uint8_t* out_level) {
	if (!counts || !out_weight || !out_level) { vdjx_set_error("vdjx_targeting_model: NULL argument"); return VDJX_EINVAL; }
	if (cls != 0 && cls != 1) { vdjx_set_error("vdjx_targeting_model: class %d (0: silent, 1: silent and replacement)", cls); return VDJX_EINVAL; }
	if (min_sub < 1 || min_mut < 1) { vdjx_set_error("vdjx_targeting_model: a minimum of 0 (both are at least 1)"); return VDJX_EINVAL; }
	// obs[m][x], opp[m][x] of the class(es); then the sums a level uses: per inner 3-mer (64), per centre (4), all
	std::vector<u64> obs(4096), opp(4096);
	for (u32 i = 0; i < 4096; i++) {
		obs[i] = counts[i] + (cls ? counts[4096 + i] : 0);
		opp[i] = counts[8192 + i] + (cls ? counts[12288 + i] : 0);
	}
	u64 a3[64][4], a1[4][4], o3[64], p3[64], o1[4], p1[4], o0 = 0, p0 = 0;
	memset(a3, 0, sizeof a3); memset(a1, 0, sizeof a1);
	memset(o3, 0, sizeof o3); memset(p3, 0, sizeof p3); memset(o1, 0, sizeof o1); memset(p1, 0, sizeof p1);
	for (u32 m = 0; m < 1024; m++) {
		const u32 in3 = (m >> 2) & 63u, ce = (m >> 4) & 3u;
		for (u32 x = 0; x < 4; x++) {
			const u64 o = obs[4 * m + x], p = opp[4 * m + x];
			a3[in3][x] += o; a1[ce][x] += o;
			o3[in3] += o; o1[ce] += o; o0 += o;
			p3[in3] += p; p1[ce] += p; p0 += p;
		}
	}
	std::vector<double> M(1024);
	for (u32 m = 0; m < 1024; m++) {
		const u32 in3 = (m >> 2) & 63u, ce = (m >> 4) & 3u;
		u64 o5 = 0, p5 = 0;
		for (u32 x = 0; x < 4; x++) { o5 += obs[4 * m + x]; p5 += opp[4 * m + x]; }
		u64 o, p;
		uint8_t lv;
		if (o5 >= min_mut && p5 > 0) { o = o5; p = p5; lv = 5; }
		else if (o3[in3] >= min_mut && p3[in3] > 0) { o = o3[in3]; p = p3[in3]; lv = 3; }
		else if (o1[ce] >= min_mut && p1[ce] > 0) { o = o1[ce]; p = p1[ce]; lv = 1; }
		else { o = o0; p = p0; lv = 0; }
		out_level[2 * m + 1] = lv;
		M[m] = o0 == 0 || p0 == 0 ? 1.0 : (double) o / (double) p;
	}
	double Z = 0.0;
	for (u32 m = 0; m < 1024; m++) Z += M[m];
	for (u32 m = 0; m < 1024; m++) {
		const u32 in3 = (m >> 2) & 63u, ce = (m >> 4) & 3u;
		u64 a[4], sum = 0;
		uint8_t lv = 5;
		for (u32 x = 0; x < 4; x++) { a[x] = obs[4 * m + x]; sum += a[x]; }
		if (sum < min_sub) {
			lv = 3; sum = 0;
			for (u32 x = 0; x < 4; x++) { a[x] = a3[in3][x]; sum += a[x]; }
		}
		if (sum < min_sub) {
			lv = 1; sum = 0;
			for (u32 x = 0; x < 4; x++) { a[x] = a1[ce][x]; sum += a[x]; }
		}
		if (sum < min_sub) {
			lv = 0; sum = 3;
			for (u32 x = 0; x < 4; x++) a[x] = x != ce;
		}
		out_level[2 * m] = lv;
		const double mz = M[m] / Z;
		for (u32 x = 0; x < 4; x++) {
			if (x == ce) { out_weight[4 * m + x] = 0; continue; }
			const double S = (double) a[x] / (double) sum;
			const double T = mz * S;
			const double scaled = T * 1e9;
			const double r = rint(scaled);
			out_weight[4 * m + x] = r < 1.0 ? 1u : (u32) r;
		}
	}
	return VDJX_OK;
}
