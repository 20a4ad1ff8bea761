// vdjx_annot.hip -- contig annotation on the device (vdjx_germline_load, vdjx_annotate; the model is in include/vdjx.h): every contig is
// scored against every V and J germline (local alignment, affine gaps), the best hits are kept, and the primary hit of each class is
// aligned again with direction bits and traced back.  Integer arithmetic throughout, no atomics on results: bitwise reproducible.
//
//   germlines    per class the records' base codes back to back, each after a reset column, one more reset column at the end
//                (d_gl_cols).  A chunk is a run of consecutive germlines of a class (at most AN_CHUNK_COLS columns).
//   phase 1      k_an_score: a wave per (contig, chunk), AN_WAVES contigs of one chunk per workgroup.  The contig's rows are striped
//                over the lanes (lane l holds rows l*R+1 .. l*R+R in registers, H and E of the column before); the chunk's columns stream
//                through as a skewed systolic pipeline: at step t lane l computes column t - l and hands the (H, F) of its last row to
//                lane l + 1 (one shift per step).  A reset column clears a lane's rows, so germlines follow each other without a new fill.
//                When a lane passes the reset column after germline k it parks its running maximum in its own slot of an LDS ring;
//                when lane 63 passes it, the whole wave reduces the slots: S of germline k, and the wave keeps the chunk's best S, how
//                many germlines hold it and the first VDJX_ANNOT_TIED of them.  k_an_merge folds the chunks of a class in index order.
//   phase 2      k_an_trace: a workgroup of one wave per primary hit recomputes the matrix by anti-diagonals (three H, two F and one E
//                diagonal in LDS), writes a direction byte per cell to the workspace (bits 0-1: where H came from -- 0 stop, 1 diagonal,
//                2 E, 3 F; bit 2: E opened here; bit 3: F opened here), finds the first cell in row-major order that holds S, and lane 0
//                walks the directions back.  (Its body, an_trace_pair, is in vdjx_align.h: vdjx_iso.hip traces contig tails with it too.)
#include "vdjx_align.h"

#include <algorithm>
#include <string.h>

#define AN_WAVES 4                       // contigs (waves) per workgroup of the scoring kernel, all over one chunk
#define AN_RING 32                       // germlines in flight per wave: each takes >= 2 columns, and a germline is in flight 64 steps
#define AN_CHUNK_COLS 65536u             // columns per chunk at most
#define AN_PAIRS 16777216u               // (contig, germline) pairs per scoring launch (VDJX_ANNOT_PAIRS)
#define AN_DIR_BYTES (256ull << 20)      // direction bytes per traceback launch

struct AnChunk { u64 col0; u32 ncols, g0, ng, cls; };

template <int R>
__global__ __launch_bounds__(64 * AN_WAVES) void k_an_score(const char* __restrict__ contigs, u32 n, int m, const uint8_t* __restrict__ cols,
                                                           const AnChunk* __restrict__ chunks, const u32* __restrict__ genes,
                                                           const uint2* __restrict__ items, AnParams p, AnBest* __restrict__ res) {
	__shared__ short ring[AN_WAVES][AN_RING][64];
	__shared__ int tl[AN_WAVES][VDJX_ANNOT_TIED];
	const u32 w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint2 it = items[blockIdx.x];
	const u32 c = it.x + w;
	if (c >= n) return;                  // (a whole wave; nothing below waits for the others)
	const AnChunk ch = chunks[it.y];
	const u32* gn = genes + ch.g0;
	const uint8_t* cc = cols + ch.col0;
	const int T = (int) ch.ncols;
	int cb[R], H[R], E[R];
#pragma unroll
	for (int r = 0; r < R; r++) {
		const int i0 = (int) lane * R + r;                // rows past m compute too: they can never hold more than a real row
		cb[r] = i0 < m ? an_ccode(contigs[(size_t) c * m + i0]) : 7;
		H[r] = 0;
		E[r] = AN_NEG;
	}
	int cur = 0, seen = 0, best = -1, ntied = 0;
	int hin = 0, fin = AN_NEG, hdiag = 0;
	int bnext = -(int) lane >= 0 && -(int) lane < T ? cc[0] : AN_SEP;
	for (int t = 0; t < T + 63; t++) {
		const int j = t - (int) lane;
		const int b = bnext;
		bnext = j + 1 >= 0 && j + 1 < T ? cc[j + 1] : AN_SEP;      // (the next step's column, loaded a step ahead)
		if (lane == 0) { hin = 0; fin = AN_NEG; hdiag = 0; }
		const bool act = j >= 0 && j < T;
		int hout = 0, fout = AN_NEG, fl = 0;
		if (act && b == AN_SEP) {
			if (seen) ring[w][(seen - 1) & (AN_RING - 1)][lane] = (short) cur;
			cur = 0;
			seen++;
			fl = seen >= 2;
#pragma unroll
			for (int r = 0; r < R; r++) { H[r] = 0; E[r] = AN_NEG; }
		} else if (act) {
			int diag = hdiag, hp = hin, fp = fin;
#pragma unroll
			for (int r = 0; r < R; r++) {
				const int s = cb[r] == b ? p.ma : -p.mi;
				const int e = max(E[r] - p.ext, H[r] - p.oe);
				const int f = max(fp - p.ext, hp - p.oe);
				const int h = max(max(diag + s, 0), max(e, f));
				diag = H[r];
				H[r] = h;
				E[r] = e;
				hp = h;
				fp = f;
				cur = max(cur, h);
			}
			hout = hp;
			fout = fp;
		}
		if (__builtin_amdgcn_readlane(fl, 63)) {              // lane 63 has passed germline k: every lane's maximum is parked
			const int k = __builtin_amdgcn_readlane(seen, 63) - 2;
			int v = ring[w][k & (AN_RING - 1)][lane];
#pragma unroll
			for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
			const int g = (int) gn[k];
			if (v > best) {
				best = v;
				ntied = 1;
				if (lane == 0) tl[w][0] = g;
			} else if (v == best) {
				if (lane == 0 && ntied < VDJX_ANNOT_TIED) tl[w][ntied] = g;
				ntied++;
			}
		}
		hdiag = hin;
		hin = __shfl_up(hout, 1, 64);
		fin = __shfl_up(fout, 1, 64);
	}
	if (lane == 0) {
		AnBest* o = res + (size_t) it.y * n + c;
		o->score = best;
		o->n_tied = ntied;
		for (int q = 0; q < VDJX_ANNOT_TIED; q++) o->tied[q] = q < ntied ? tl[w][q] : -1;
	}
}

// one thread per (contig, class): the class's chunks in index order; the call when S reaches the class's minimum
__global__ void k_an_merge(const AnBest* __restrict__ res, u32 n, uint2 ck_v, uint2 ck_j, int min_v, int min_j, vdjx_annot_hit* __restrict__ hits) {
	const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= 2 * n) return;
	const u32 c = q >> 1, cls = q & 1u;
	const uint2 ck = cls ? ck_j : ck_v;
	int best = -1, nt = 0, tied[VDJX_ANNOT_TIED];
	for (u32 k = ck.x; k < ck.y; k++) {
		const AnBest b = res[(size_t) k * n + c];
		if (b.score > best) { best = b.score; nt = 0; }
		if (b.score == best) {
			for (int z = 0; z < b.n_tied && z < VDJX_ANNOT_TIED; z++)
				if (nt + z < VDJX_ANNOT_TIED) tied[nt + z] = b.tied[z];
			nt += b.n_tied;
		}
	}
	vdjx_annot_hit* h = hits + (size_t) cls * n + c;
	const int mn = cls ? min_j : min_v;
	h->score = best < 0 ? 0 : best;
	if (best < 0 || best < mn) {
		h->gene = -1;
		for (int z = 0; z < VDJX_ANNOT_TIED; z++) h->tied[z] = -1;
		return;
	}
	h->gene = tied[0];
	h->n_tied = nt;
	for (int z = 0; z < VDJX_ANNOT_TIED; z++) h->tied[z] = z < nt ? tied[z] : -1;
}

#define AN_TMAX 4096
__global__ __launch_bounds__(64) void k_an_trace(const char* __restrict__ contigs, int m, const uint8_t* __restrict__ cols,
                                                 const AnAlign* __restrict__ al, AnParams p, uint8_t* __restrict__ dirs, u32 n,
                                                 vdjx_annot_hit* __restrict__ hits) {
	__shared__ short Hb[3][AN_TMAX], Fb[2][AN_TMAX], Eb[AN_TMAX];
	const AnAlign a = al[blockIdx.x];
	an_trace_pair(contigs + (size_t) a.contig * m, m, cols + a.gat, a.g, p, dirs + a.dir, hits + (size_t) a.cls * n + a.contig, 0, &Hb[0][0], &Fb[0][0],
	              Eb, AN_TMAX);
}

static u32 an_pairs_knob() {
	static const u32 v = (u32) vdjx_env_num("VDJX_ANNOT_PAIRS", AN_PAIRS, 1, 0xFFFFFFFFll);
	return v;
}

extern "C" int vdjx_germline_load(vdjx_ctx* c, const char* seqs, const uint64_t* off, const char* cls, size_t n) {
	if (!c || (n && (!seqs || !off || !cls))) { vdjx_set_error("vdjx_germline_load: NULL argument"); return VDJX_EINVAL; }
	if (n >= (1ull << 20)) { vdjx_set_error("vdjx_germline_load: %zu records (at most 2^20 - 1)", n); return VDJX_EINVAL; }
	std::vector<u32> gene[2], glen[2];
	u64 total[2] = {0, 0};
	for (size_t r = 0; r < n; r++) {
		const int k = cls[r] == 'V' ? 0 : cls[r] == 'J' ? 1 : -1;
		if (off[r + 1] < off[r]) { vdjx_set_error("vdjx_germline_load: offsets of record %zu decrease", r); return VDJX_EINVAL; }
		if (k < 0) continue;
		const u64 L = off[r + 1] - off[r];
		if (L == 0 || L >= 2048) { vdjx_set_error("vdjx_germline_load: record %zu has %llu bases (1 .. 2047)", r, (unsigned long long) L); return VDJX_EINVAL; }
		gene[k].push_back((u32) r);
		glen[k].push_back((u32) L);
		total[k] += L + 1;
	}
	c->gl_loaded = false;
	std::vector<uint8_t> h;
	h.reserve(total[0] + total[1] + 2);
	for (int k = 0; k < 2; k++) {
		c->gl_class_at[k] = h.size();
		c->gl_at[k].clear();
		for (size_t q = 0; q < gene[k].size(); q++) {
			c->gl_at[k].push_back(h.size());
			h.push_back(AN_SEP);
			const u64 r = gene[k][q];
			for (u64 x = off[r]; x < off[r + 1]; x++) h.push_back(an_gcode(seqs[x]));
		}
		c->gl_at[k].push_back(h.size());
		h.push_back(AN_SEP);
		c->gl_gene[k] = gene[k];
		c->gl_len[k] = glen[k];
	}
	c->gl_class_at[2] = h.size();
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (h.size() > c->gl_cols_cap) {
		if (c->d_gl_cols) HIP_TRY(hipFree(c->d_gl_cols));
		c->d_gl_cols = nullptr;
		c->gl_cols_cap = 0;
		HIP_TRY(hipMalloc(&c->d_gl_cols, h.size()));
		c->gl_cols_cap = h.size();
	}
	HIP_TRY(hipMemcpy(c->d_gl_cols, h.data(), h.size(), hipMemcpyHostToDevice));
	c->gl_loaded = true;
	return VDJX_OK;
}

template <int R>
static void an_launch_score(u32 blocks, hipStream_t st, const char* ct, u32 n, int m, const uint8_t* cols, const AnChunk* ck, const u32* genes,
                            const uint2* items, AnParams p, AnBest* res) {
	hipLaunchKernelGGL(k_an_score<R>, dim3(blocks), dim3(64 * AN_WAVES), 0, st, ct, n, m, cols, ck, genes, items, p, res);
}

static int an_rows(int m) {                 // rows per lane: the smallest instantiated R with 64 R >= m
	static const int rs[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64};
	for (int r : rs)
		if (64 * r >= m) return r;
	return 64;
}

static double an_us_since(std::chrono::steady_clock::time_point t) {
	return (double) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t).count();
}

extern "C" int vdjx_annotate(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_annot_params* prm, vdjx_annot_hit* out_v,
                             vdjx_annot_hit* out_j) {
	if (!c || !prm || (n && (!contigs || !out_v || !out_j))) { vdjx_set_error("vdjx_annotate: NULL argument"); return VDJX_EINVAL; }
	if (prm->match < 1 || prm->match > 15 || prm->mismatch < 0 || prm->mismatch > 31 || prm->gap_open < 0 || prm->gap_open > 31 ||
	    prm->gap_extend < 0 || prm->gap_extend > 31) {
		vdjx_set_error("vdjx_annotate: parameters match=%d mismatch=%d gap_open=%d gap_extend=%d (match 1..15, the others 0..31)", prm->match,
		               prm->mismatch, prm->gap_open, prm->gap_extend);
		return VDJX_EINVAL;
	}
	if (!c->gl_loaded) { vdjx_set_error("vdjx_annotate: no germline set is loaded (call vdjx_germline_load first)"); return VDJX_ESTATE; }
	c->stats["annot_cells"] = 0;
	c->stats["annot_score_us"] = 0;
	c->stats["annot_trace_us"] = 0;
	c->stats["annot_cigar_truncated"] = 0;
	if (n == 0) return VDJX_OK;
	if (len < 1 || len >= 4096) { vdjx_set_error("vdjx_annotate: len=%d (1 .. 4095)", len); return VDJX_EINVAL; }
	if (n >= (1ull << 20)) { vdjx_set_error("vdjx_annotate: %zu contigs (at most 2^20 - 1 per call)", n); return VDJX_EINVAL; }
	if (memchr(contigs, 0, n * (size_t) len)) { vdjx_set_error("vdjx_annotate: contigs of unequal length (a NUL inside the %zu x %d characters)", n, len); return VDJX_EINVAL; }
	const auto t0 = std::chrono::steady_clock::now();
	const AnParams p = {prm->match, prm->mismatch, prm->gap_open + prm->gap_extend, prm->gap_extend};
	const u32 pairs = an_pairs_knob();
	const u32 per_chunk = std::max<u32>(1u, pairs / AN_WAVES);

	// chunks: V's, then J's; items: chunk-major, AN_WAVES contigs each
	std::vector<AnChunk> chunks;
	std::vector<u32> genes;
	uint2 ck[2];
	u64 cells = 0;
	for (int k = 0; k < 2; k++) {
		ck[k].x = (u32) chunks.size();
		const u32 g0 = (u32) genes.size(), ng = (u32) c->gl_gene[k].size();
		genes.insert(genes.end(), c->gl_gene[k].begin(), c->gl_gene[k].end());
		for (u32 a = 0; a < ng;) {
			u32 b = a + 1;
			while (b < ng && b - a < per_chunk && c->gl_at[k][b + 1] - c->gl_at[k][a] + 1 <= AN_CHUNK_COLS) b++;
			chunks.push_back({c->gl_at[k][a], (u32) (c->gl_at[k][b] - c->gl_at[k][a] + 1), g0 + a, b - a, (u32) k});
			a = b;
		}
		ck[k].y = (u32) chunks.size();
		for (u32 x : c->gl_len[k]) cells += (u64) x * (u64) len * (u64) n;
	}
	const u32 ngroups = (u32) ((n + AN_WAVES - 1) / AN_WAVES);
	std::vector<uint2> items;
	std::vector<u32> launch_at{0};
	u64 acc = 0;
	for (u32 q = 0; q < (u32) chunks.size(); q++)
		for (u32 gr = 0; gr < ngroups; gr++) {
			const u64 pp = (u64) std::min<u64>(AN_WAVES, n - (u64) gr * AN_WAVES) * chunks[q].ng;
			if (acc && acc + pp > pairs) { launch_at.push_back((u32) items.size()); acc = 0; }
			items.push_back(make_uint2(gr * AN_WAVES, q));
			acc += pp;
		}
	launch_at.push_back((u32) items.size());

	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	vdjx_work wk(c);
	char* d_ct;
	AnChunk* d_ck;
	u32* d_genes;
	uint2* d_items;
	AnBest* d_res;
	vdjx_annot_hit* d_hits;
	const size_t nck = chunks.size();
	HIP_TRY(wk.alloc(&d_ct, n * (size_t) len));
	HIP_TRY(wk.alloc(&d_ck, nck));
	HIP_TRY(wk.alloc(&d_genes, genes.size()));
	HIP_TRY(wk.alloc(&d_items, items.size()));
	HIP_TRY(wk.alloc(&d_res, nck * n));
	HIP_TRY(wk.alloc(&d_hits, 2 * n));
	HIP_TRY(hipMemcpyAsync(d_ct, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
	if (nck) HIP_TRY(hipMemcpyAsync(d_ck, chunks.data(), nck * sizeof(AnChunk), hipMemcpyHostToDevice, st));
	if (!genes.empty()) HIP_TRY(hipMemcpyAsync(d_genes, genes.data(), genes.size() * 4, hipMemcpyHostToDevice, st));
	if (!items.empty()) HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_hits, 0, 2 * n * sizeof(vdjx_annot_hit), st));
	const int R = an_rows(len);
	{
		vdjx_prof_scope ps(c, "k_annot_score");
		for (size_t L = 0; L + 1 < launch_at.size(); L++) {
			const u32 b0 = launch_at[L], nb = launch_at[L + 1] - b0;
			if (!nb) continue;
			const uint2* itp = d_items + b0;
			switch (R) {
#define AN_CASE(RR) case RR: an_launch_score<RR>(nb, st, d_ct, (u32) n, len, c->d_gl_cols, d_ck, d_genes, itp, p, d_res); break;
				AN_CASE(1) AN_CASE(2) AN_CASE(3) AN_CASE(4) AN_CASE(6) AN_CASE(8) AN_CASE(12) AN_CASE(16) AN_CASE(24) AN_CASE(32) AN_CASE(48) AN_CASE(64)
#undef AN_CASE
			}
		}
		hipLaunchKernelGGL(k_an_merge, dim3((u32) ((2 * n + 255) / 256)), dim3(256), 0, st, (const AnBest*) d_res, (u32) n, ck[0], ck[1],
		                   prm->min_v_score, prm->min_j_score, d_hits);
	}
	std::vector<vdjx_annot_hit> hh(2 * n);
	HIP_TRY(hipMemcpyAsync(hh.data(), d_hits, 2 * n * sizeof(vdjx_annot_hit), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	const double us_score = an_us_since(t0);
	const auto t1 = std::chrono::steady_clock::now();

	// phase 2: the primary hits with S > 0, in launches of at most AN_DIR_BYTES direction bytes
	std::vector<AnAlign> al;
	std::vector<u64> dir_need;
	for (int k = 0; k < 2; k++)
		for (size_t q = 0; q < n; q++) {
			const vdjx_annot_hit& h = hh[(size_t) k * n + q];
			if (h.gene < 0 || h.score <= 0) continue;
			const u32 slot = (u32) (std::lower_bound(c->gl_gene[k].begin(), c->gl_gene[k].end(), (u32) h.gene) - c->gl_gene[k].begin());
			const int g = (int) c->gl_len[k][slot];
			al.push_back({(u32) q, (u32) k, 0, c->gl_at[k][slot], g});
		}
	if (!al.empty()) {
		AnAlign* d_al;
		uint8_t* d_dir;
		u64 maxb = 0;
		for (auto& a : al) maxb = std::max<u64>(maxb, (u64) len * (u64) a.g);
		const u64 cap = std::max<u64>(AN_DIR_BYTES, maxb);
		HIP_TRY(wk.alloc(&d_al, al.size()));
		HIP_TRY(wk.alloc(&d_dir, cap));
		std::vector<size_t> at{0};
		u64 used = 0;
		for (size_t x = 0; x < al.size(); x++) {
			const u64 b = (u64) len * (u64) al[x].g;
			if (used && used + b > cap) { at.push_back(x); used = 0; }
			al[x].dir = used;
			used += b;
		}
		at.push_back(al.size());
		HIP_TRY(hipMemcpyAsync(d_al, al.data(), al.size() * sizeof(AnAlign), hipMemcpyHostToDevice, st));
		vdjx_prof_scope ps(c, "k_annot_trace");
		for (size_t L = 0; L + 1 < at.size(); L++)
			hipLaunchKernelGGL(k_an_trace, dim3((u32) (at[L + 1] - at[L])), dim3(64), 0, st, (const char*) d_ct, len, (const uint8_t*) c->d_gl_cols,
			                   (const AnAlign*) d_al + at[L], p, d_dir, (u32) n, d_hits);
	}
	HIP_TRY(hipMemcpyAsync(out_v, d_hits, n * sizeof(vdjx_annot_hit), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(out_j, d_hits + n, n * sizeof(vdjx_annot_hit), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	vdjx_prof_collect(c, false);
	u64 trunc = 0;
	for (size_t q = 0; q < n; q++) trunc += (out_v[q].n_runs > VDJX_ANNOT_RUNS) + (out_j[q].n_runs > VDJX_ANNOT_RUNS);
	c->stats["annot_cells"] = cells;
	c->stats["annot_score_us"] = (uint64_t) us_score;
	c->stats["annot_trace_us"] = (uint64_t) an_us_since(t1);
	c->stats["annot_cigar_truncated"] = trunc;
	return VDJX_OK;
}
