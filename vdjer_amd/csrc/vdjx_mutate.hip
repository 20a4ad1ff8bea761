// vdjx_mutate.hip -- germline rows and R/S mutation counts (gfx950 only, wave64).
//
//   vdjx_mutations_layout   host only: every contig's columns from the hits alone
//   vdjx_mutations          lays each contig and its V(D)J germline side by side, column by column, and classifies the V differences codon
//                           by codon (the model: include/vdjx.h; in Python: tests/mutation_model.py)
//
// The hits are the caller's, so the host checks every one of them before anything reaches the device (vh_check of vdjx_vhit.h, then mu_plan):
// every index the kernel forms lies inside the contig, the record and the row buffers because the run lengths were summed there.  Per contig
// the host uploads 64 bytes of positions and record offsets (MuContig) and the usable hits' runs, 4 bytes each.  The hit check, a hit's rows
// of the segment table and the codon resolver are vdjx_vhit.h's, shared with vdjx_select.hip; what is here is the layout, the rows pass and
// what a resolved codon counts as.
//   k_mutations   one dispatch; a wave per contig, MU_WAVES waves per workgroup, no barrier between the waves.
//     table       one lane per run of V, then of D, then of J (vh_hit_segments per hit) gives the segment table in LDS: MU_SLOTS segments
//                 {first column, first contig index, first germline column, op | region << 2} in a fixed order -- V's runs 0 .. 63, np1 64,
//                 D's runs 65 .. 128, np2 129, J's runs 130 .. 193.  A slot without a run is empty at its section's end, so the first
//                 columns (and, inside V, the germline columns) ascend over the whole table and the segment of a column is the LAST slot
//                 that starts at or before it.  A clipped J loses its first jdrop columns.
//     rows        the columns are striped over the lanes (column = lane + 64 k); a lane finds its segment by a binary search of the table,
//                 reads its contig character and germline code and writes one byte of each row: 64 consecutive bytes per store.  It counts
//                 the V M columns below the limit that mismatch, and J's mismatches.
//     codons      a lane per V germline codon; its three bases go to columns through the same table (vh_codon: searched by germline
//                 column); a classifiable codon's differences are classified through a 64-entry amino-acid table in LDS.
//     row         the counts are reduced across the wave by shuffles (v_na = the mismatches below the limit - the classified ones); lane 0
//                 writes the 32-byte row as two 16-byte stores.
// No floating point, no atomics, no scratch.
#include "vdjx_vhit.h"

#define MU_WAVES 4
#define MU_V0 0
#define MU_NP1 64
#define MU_D0 65
#define MU_NP2 129
#define MU_J0 130
#define MU_SLOTS 194
#define MU_OP_N 3                        // a gap column: (contig base, 'N')

struct MuContig {
	u64 out_off;                         // where the contig's rows start in each row buffer
	u32 run_off;                         // its runs in the pool: V's, then D's, then J's
	u32 v_at, d_at, j_at;                // the column of the hit's base germ_start in its set's columns
	u32 nruns;                           // V's | D's << 8 | J's << 16
	u32 flags;
	int v_seq0, d_seq0, j_seq0;          // seq_start - 1 of the hits
	int v_germ0;                         // V's germ_start - 1
	int gap, np1;                        // contig bases between V and the kept J; those of them before D (all of them without D)
	int jdrop;                           // J's columns dropped at its 5' end
	int limit;
};
static_assert(sizeof(MuContig) == 64 && sizeof(vdjx_mut_row) == 32 && sizeof(vdjx_mut_info) == 72, "uploaded / returned as they are");

__global__ __launch_bounds__(64 * MU_WAVES) void k_mutations(const char* __restrict__ contigs, u32 n, u32 len, const MuContig* __restrict__ mc,
                                                            const u32* __restrict__ runs, const uint8_t* __restrict__ gcols,
                                                            const uint8_t* __restrict__ dcols, char* __restrict__ out_seq,
                                                            char* __restrict__ out_germ, char* __restrict__ out_mask, int4* __restrict__ out_rows) {
	__shared__ int4 seg_all[MU_WAVES][MU_SLOTS];
	__shared__ char aa_all[MU_WAVES][64];
	const u32 w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const u32 c = blockIdx.x * MU_WAVES + w;
	if (c >= n) return;                  // (a whole wave; nothing below waits for the others)
	int4* seg = seg_all[w];
	char* aa = aa_all[w];
	aa[lane] = vh_aa[lane];
	const MuContig q = mc[c];
	const char* ct = contigs + (size_t) c * len;
	const int nr[3] = {(int) (q.nruns & 255u), (int) (q.nruns >> 8 & 255u), (int) (q.nruns >> 16 & 255u)};
	const int slot0[3] = {MU_V0, MU_D0, MU_J0};
	const int seq0[3] = {q.v_seq0, q.d_seq0, q.j_seq0};
	const u32 at0[3] = {q.v_at, q.d_at, q.j_at};
	int colbase = 0, vgerm = 0, roff = 0;
#pragma unroll
	for (int h = 0; h < 3; h++) {
		const int drop = h == 2 ? q.jdrop : 0;
		int tc, tb, tg;
		seg[slot0[h] + (int) lane] = vh_hit_segments(runs, q.run_off + (u32) roff, nr[h], lane, colbase, seq0[h], (int) at0[h], drop, h, tc, tb, tg);
		colbase += tc - drop;
		roff += nr[h];
		if (h == 0) {
			vgerm = tg;
			if (lane == 0) seg[MU_NP1] = make_int4(colbase, q.v_seq0 + tb, 0, MU_OP_N | 4);
			colbase += q.np1;
		}
		if (h == 1) {
			const int np2 = q.gap - q.np1 - tb;
			if (lane == 0) seg[MU_NP2] = make_int4(colbase, q.d_seq0 + tb, 0, MU_OP_N | 4);
			colbase += np2;
		}
	}
	const int cols = colbase;
	vdjx_wave_lds_fence();               // the table and the amino acids are read by other lanes of the wave

	// the rows
	const bool wr = out_seq || out_germ || out_mask;
	int vmis = 0, jmis = 0;
	for (int col = (int) lane; col < cols; col += 64) {
		int lo = 0, hi = MU_SLOTS;           // the last slot whose first column is <= col (slot 0 starts at column 0)
		while (hi - lo > 1) {
			const int mid = (lo + hi) >> 1;
			if (seg[mid].x <= col) lo = mid; else hi = mid;
		}
		const int4 s = seg[lo];
		const int off = col - s.x, op = s.w & 3, region = s.w >> 2;
		char a = '-', g = '-';
		int code = 5;
		if (op != 2) a = ct[s.y + off];
		if (op == MU_OP_N) g = 'N';
		else if (op != 1) {
			code = (region == 1 ? dcols : gcols)[(u32) s.z + (u32) off];
			g = code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : code == 3 ? 'T' : 'N';
		}
		if (op == 0 && vh_ccode(a) != code) {
			if (region == 0 && s.y + off < q.limit) vmis++;
			if (region == 2) jmis++;
		}
		if (wr) {
			const size_t o = (size_t) q.out_off + (size_t) col;
			if (out_seq) out_seq[o] = a;
			if (out_germ) out_germ[o] = g;
			if (out_mask) out_mask[o] = region == 1 ? 'N' : g;
		}
	}

	// the codons of the record that lie inside germ_start .. germ_end
	int vr = 0, vs = 0, vstop = 0, ncod = 0;
	int c_lo, c_hi;
	vh_codon_range(q.v_germ0, vgerm, c_lo, c_hi);
	for (int cd = c_lo + (int) lane; cd < c_hi; cd += 64) {
		int cb[3], gb[3];
		if (!vh_codon(seg, ct, gcols, q.v_at, q.v_germ0, q.limit, cd, cb, gb)) continue;
		ncod++;
		const int gc = 16 * gb[0] + 4 * gb[1] + gb[2];
		const char ga_ = aa[gc];
#pragma unroll
		for (int b = 0; b < 3; b++) {
			if (cb[b] == gb[b]) continue;
			const char ma = vh_subst_aa(aa, gc, b, cb[b]);
			if (ga_ == '*' || ma == '*') vstop++;
			else if (ga_ == ma) vs++;
			else vr++;
		}
	}
	vmis = vdjx_wave_sum(vmis);
	jmis = vdjx_wave_sum(jmis);
	vr = vdjx_wave_sum(vr);
	vs = vdjx_wave_sum(vs);
	vstop = vdjx_wave_sum(vstop);
	ncod = vdjx_wave_sum(ncod);
	if (lane == 0) {
		out_rows[2 * (size_t) c] = make_int4(cols, vr, vs, vstop);
		out_rows[2 * (size_t) c + 1] = make_int4(vmis - vr - vs - vstop, ncod, jmis, (int) q.flags);
	}
}

// ---- the host's side: the checks and the layout ----------------------------------------------------------------------------------------
struct MuPlan { u32 flags; u32 truncated; int64_t cols; int jdrop, gap, np1; bool use_d; };

// contig i's plan from its hits alone (d may be NULL); false: a run with an op outside 0..2 or a length of 0
static bool mu_plan(const vdjx_annot_hit& v, const vdjx_annot_hit* d, const vdjx_annot_hit& j, MuPlan& p) {
	memset(&p, 0, sizeof p);
	p.truncated = (u32) (vh_called(v) && !vh_usable(v)) + (u32) (vh_called(j) && !vh_usable(j)) + (u32) (d && vh_called(*d) && !vh_usable(*d));
	if (p.truncated) p.flags |= 16;
	int64_t vc, vs, vg, jc = 0, js = 0, jg = 0, dc = 0, ds = 0, dg = 0;
	if (vh_usable(v) && !vh_run_sums(v, vc, vs, vg)) return false;
	if (vh_usable(j) && !vh_run_sums(j, jc, js, jg)) return false;
	if (d && vh_usable(*d) && !vh_run_sums(*d, dc, ds, dg)) return false;
	if (!vh_usable(v)) return true;
	p.flags |= 1;
	p.cols = vc;
	if (!vh_usable(j)) return true;
	int64_t kept = jc;
	if (j.seq_start <= v.seq_end) {          // clipped: up to the column of contig position v.seq_end + 1
		p.flags |= 8;
		int64_t col = 0, pos = j.seq_start;
		kept = 0;
		for (int r = 0; r < j.n_runs; r++) {
			const int64_t L = j.runs[r] >> 4;
			const u32 op = j.runs[r] & 15u;
			if (op != 2 && pos + L > (int64_t) v.seq_end + 1) {
				p.jdrop = (int) (col + ((int64_t) v.seq_end + 1 - pos));
				kept = jc - p.jdrop;
				break;
			}
			col += L;
			if (op != 2) pos += L;
		}
		if (!kept) return true;              // (J lies inside V: not used)
	} else p.gap = j.seq_start - 1 - v.seq_end;
	p.flags |= 2;
	p.np1 = p.gap;
	if (d && vh_usable(*d) && d->seq_start > v.seq_end && d->seq_end <= v.seq_end + p.gap) {
		p.flags |= 4;
		p.use_d = true;
		p.np1 = d->seq_start - v.seq_end - 1;
		p.cols += dc - ds;                   // (its D columns: the gap's contig bases are counted below)
	}
	p.cols += p.gap + kept;
	return true;
}

extern "C" int vdjx_mutations_layout(const vdjx_annot_hit* v, const vdjx_annot_hit* d, const vdjx_annot_hit* j, size_t n, uint64_t* out_off) {
	if (!out_off || (n && (!v || !j))) { vdjx_set_error("vdjx_mutations_layout: NULL argument"); return VDJX_EINVAL; }
	out_off[0] = 0;
	for (size_t i = 0; i < n; i++) {
		MuPlan p;
		if (!mu_plan(v[i], d ? d + i : nullptr, j[i], p)) {
			vdjx_set_error("vdjx_mutations_layout: a hit of contig %zu has a run with an op outside 0..2 or a length of 0", i);
			return VDJX_EINVAL;
		}
		out_off[i + 1] = out_off[i] + (u64) p.cols;
	}
	return VDJX_OK;
}

// a usable hit of contig i against its record set: *at = the column of its base germ_start.  what: "V", "D", "J"
static int mu_check(const char* what, size_t i, const vdjx_annot_hit& h, const vdjx_recset& s, int cls, int len, u32* at) {
	size_t slot = 0;
	const int rc = vh_check("vdjx_mutations", what, i, h, s, cls, len, &slot);
	if (rc == VDJX_OK) *at = (u32) (s.at[cls][slot] + (u64) h.germ_start);      // (at: the record's reset column; its base 1 follows)
	return rc;
}

extern "C" int vdjx_mutations(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_annot_hit* v, const vdjx_annot_hit* d,
                              const vdjx_annot_hit* j, const int32_t* limit, char* out_seq, char* out_germ, char* out_mask,
                              vdjx_mut_row* out_rows, vdjx_mut_info* info) {
	if (info) memset(info, 0, sizeof *info);
	if (!c) { vdjx_set_error("vdjx_mutations: NULL argument"); return VDJX_EINVAL; }
	if (n == 0) return VDJX_OK;
	if (!contigs || !v || !j || !out_rows) { vdjx_set_error("vdjx_mutations: NULL argument"); return VDJX_EINVAL; }
	int rc = vh_check_sizes("vdjx_mutations", n, len);
	if (rc == VDJX_OK) rc = vh_check_contigs("vdjx_mutations", c, contigs, n, len);
	if (rc != VDJX_OK) return rc;
	if (d && !c->dsegment.loaded) { vdjx_set_error("vdjx_mutations: D hits are given and no D set is loaded (call vdjx_dsegment_load first)"); return VDJX_ESTATE; }
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<MuContig> mc(n);
	std::vector<u32> runs;
	u64 total = 0;
	u32 truncated = 0;
	for (size_t i = 0; i < n; i++) {
		const int lim = limit ? limit[i] : len;
		if (lim < 0 || lim > len) { vdjx_set_error("vdjx_mutations: contig %zu: limit %d (0 .. %d)", i, lim, len); return VDJX_EINVAL; }
		MuContig& q = mc[i];
		memset(&q, 0, sizeof q);
		u32 at[3] = {0, 0, 0};
		rc = VDJX_OK;
		if (vh_usable(v[i])) rc = mu_check("V", i, v[i], c->germline, 0, len, &at[0]);
		if (rc == VDJX_OK && d && vh_usable(d[i])) rc = mu_check("D", i, d[i], c->dsegment, 0, len, &at[1]);
		if (rc == VDJX_OK && vh_usable(j[i])) rc = mu_check("J", i, j[i], c->germline, 1, len, &at[2]);
		if (rc != VDJX_OK) return rc;
		MuPlan p;
		mu_plan(v[i], d ? d + i : nullptr, j[i], p);          // (the runs passed mu_check)
		truncated += p.truncated;
		q.out_off = total;
		q.run_off = (u32) runs.size();
		q.flags = p.flags;
		q.limit = lim;
		total += (u64) p.cols;
		if (!(p.flags & 1)) continue;
		u32 nv = (u32) v[i].n_runs, nd = 0, nj = 0;
		runs.insert(runs.end(), v[i].runs, v[i].runs + nv);
		q.v_at = at[0];
		q.v_seq0 = v[i].seq_start - 1;
		q.v_germ0 = v[i].germ_start - 1;
		q.d_seq0 = q.j_seq0 = v[i].seq_end;                   // (unused sections sit empty at V's end)
		if (p.use_d) {
			nd = (u32) d[i].n_runs;
			runs.insert(runs.end(), d[i].runs, d[i].runs + nd);
			q.d_at = at[1];
			q.d_seq0 = d[i].seq_start - 1;
		}
		if (p.flags & 2) {
			nj = (u32) j[i].n_runs;
			runs.insert(runs.end(), j[i].runs, j[i].runs + nj);
			q.j_at = at[2];
			q.j_seq0 = j[i].seq_start - 1;
			q.gap = p.gap;
			q.np1 = p.np1;
			q.jdrop = p.jdrop;
		}
		q.nruns = nv | nd << 8 | nj << 16;
	}

	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	vdjx_work wk(c);
	char *d_ct, *d_rows3;
	MuContig* d_mc;
	u32* d_runs;
	int4* d_out;
	const bool want[3] = {out_seq != nullptr, out_germ != nullptr, out_mask != nullptr};
	const size_t nwant = (size_t) want[0] + want[1] + want[2];
	HIP_TRY(wk.alloc(&d_ct, n * (size_t) len));
	HIP_TRY(wk.alloc(&d_mc, n));
	HIP_TRY(wk.alloc(&d_runs, runs.size()));
	HIP_TRY(wk.alloc(&d_rows3, nwant * total));
	HIP_TRY(wk.alloc(&d_out, 2 * n));
	HIP_TRY(hipMemcpyAsync(d_ct, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_mc, mc.data(), n * sizeof(MuContig), hipMemcpyHostToDevice, st));
	if (!runs.empty()) HIP_TRY(hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(u32), hipMemcpyHostToDevice, st));
	char* d_row[3];
	for (size_t k = 0, used = 0; k < 3; k++) d_row[k] = want[k] && total ? d_rows3 + total * used++ : nullptr;
	{
		vdjx_prof_scope ps(c, "k_mutations");
		hipLaunchKernelGGL(k_mutations, dim3((u32) ((n + MU_WAVES - 1) / MU_WAVES)), dim3(64 * MU_WAVES), 0, st, (const char*) d_ct, (u32) n, (u32) len,
		                   (const MuContig*) d_mc, (const u32*) d_runs, (const uint8_t*) c->germline.d_cols,
		                   (const uint8_t*) (d ? c->dsegment.d_cols : c->germline.d_cols), d_row[0], d_row[1], d_row[2], d_out);
	}
	char* const host_row[3] = {out_seq, out_germ, out_mask};
	for (int k = 0; k < 3; k++)
		if (d_row[k]) HIP_TRY(hipMemcpyAsync(host_row[k], d_row[k], total, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(out_rows, d_out, n * sizeof(vdjx_mut_row), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	vdjx_prof_collect(c, false);
	if (info) {
		info->contigs = n;
		info->truncated = truncated;
		for (size_t i = 0; i < n; i++) {
			const vdjx_mut_row& r = out_rows[i];
			info->aligned += (r.flags & 1) != 0;
			info->clipped += (r.flags & 8) != 0;
			info->cols += (u64) r.cols;
			info->v_r += (u64) r.v_r;
			info->v_s += (u64) r.v_s;
			info->v_stop += (u64) r.v_stop;
			info->v_na += (u64) r.v_na;
			info->v_codons += (u64) r.v_codons;
		}
	}
	c->stats["mutations_cols"] = total;
	c->stats["mutations_us"] = (u64) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
	return VDJX_OK;
}
