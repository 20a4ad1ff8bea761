// vdjx_iso.hip -- isotype calls on the device (vdjx_constant_load, vdjx_isotype; the model is in include/vdjx.h): the last T bases of every
// contig are scored against every constant-region record (vdjx_annotate's local alignment, unchanged), every score is kept, the best
// record is called and aligned again with direction bits and traced back.  Integer arithmetic, no atomics: bitwise reproducible.
//
//   constants    the records' base codes back to back, each after a reset column, one more reset column at the end (d_cs_cols).  A chunk
//                is a run of consecutive records of at most ISO_CHUNK_COLS columns (one record at least).
//   phase 1      k_iso_score: a wave per (contig, chunk), ISO_WAVES contigs of one chunk per workgroup.  Lane l owns tail row l + 1: H and E
//                of the column before stay in its registers, and the chunk's columns stream through by anti-diagonals -- at step t lane l
//                computes column t - l and hands its (H, F) to lane l + 1 by one lane shift each; the diagonal H is the H that arrived a
//                step earlier.  A reset column clears a lane's row, so the records of a chunk follow each other and the T-step fill is
//                paid per chunk, not per record.  A lane that passes the reset column after record k parks its running maximum in its slot
//                of an LDS ring; when lane 63 passes it the wave folds the 64 slots by a fixed butterfly: S(contig, k), written to the
//                score matrix, and the chunk's best S, tie count and first VDJX_ANNOT_TIED ties are kept in index order.
//                k_iso_merge folds the chunks in index order and makes the call.
//   phase 2      k_iso_trace: vdjx_annot.hip's traceback (an_trace_pair, vdjx_align.h) of the tail against the primary hit, its
//                coordinates moved to the contig's.
#include "vdjx_align.h"

#include <algorithm>
#include <string.h>

#define ISO_WAVES 4                      // contigs (waves) per workgroup of the scoring kernel, all over one chunk
#define ISO_RING 32                      // records in flight per wave: each takes >= 2 columns, and a record is in flight 64 steps
#define ISO_CHUNK_COLS 2304u             // columns per chunk at most (a record of 2047 bases and its two reset columns fit)
#define ISO_DIR_BYTES (256ull << 20)     // direction bytes per traceback launch
#define ISO_TSTRIDE 66                   // shorts between the traceback's LDS diagonals (rows 0 .. 64)
#define ISO_MAX_RECORDS 4096u

struct IsoChunk { u64 col0; u32 ncols, r0, nr; };

__global__ __launch_bounds__(64 * ISO_WAVES) void k_iso_score(const char* __restrict__ contigs, u32 n, int len, int T,
                                                             const uint8_t* __restrict__ cols, const IsoChunk* __restrict__ chunks, u32 C,
                                                             AnParams p, int* __restrict__ scores, AnBest* __restrict__ res) {
	__shared__ short ring[ISO_WAVES][ISO_RING][64];
	__shared__ int tl[ISO_WAVES][VDJX_ANNOT_TIED];
	const u32 w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const u32 c = blockIdx.x * ISO_WAVES + w;
	if (c >= n) return;                  // (a whole wave; nothing below waits for the others)
	const IsoChunk ch = chunks[blockIdx.y];
	const uint8_t* cc = cols + ch.col0;
	const int NC = (int) ch.ncols;
	const bool row = (int) lane < T;     // lanes past the tail compute too (a base that matches nothing); their maxima are not counted
	const int cb = row ? an_ccode(contigs[(size_t) c * len + (len - T) + lane]) : 7;
	int H = 0, E = AN_NEG;               // this row's H and E of the column before
	int cur = 0, seen = 0, best = -1, ntied = 0;
	int hin = 0, fin = AN_NEG, hdiag = 0;
	int bnext = lane == 0 ? cc[0] : AN_SEP;
	for (int t = 0; t < NC + 63; t++) {
		const int j = t - (int) lane;
		const int b = bnext;
		bnext = j + 1 >= 0 && j + 1 < NC ? cc[j + 1] : AN_SEP;         // (the next step's column, loaded a step ahead)
		if (lane == 0) { hin = 0; fin = AN_NEG; hdiag = 0; }
		const bool act = j >= 0 && j < NC;
		int hout = 0, fout = AN_NEG, fl = 0;
		if (act && b == AN_SEP) {
			if (seen) ring[w][(seen - 1) & (ISO_RING - 1)][lane] = (short) cur;
			cur = 0;
			seen++;
			fl = seen >= 2;
			H = 0;
			E = AN_NEG;
		} else if (act) {
			const int s = cb == b ? p.ma : -p.mi;
			const int e = max(E - p.ext, H - p.oe);
			const int f = max(fin - p.ext, hin - p.oe);
			const int h = max(max(hdiag + s, 0), max(e, f));
			H = h;
			E = e;
			cur = max(cur, row ? h : 0);
			hout = h;
			fout = f;
		}
		if (__builtin_amdgcn_readlane(fl, 63)) {                  // lane 63 has passed record k: every lane's maximum is parked
			const int k = __builtin_amdgcn_readlane(seen, 63) - 2;
			int v = ring[w][k & (ISO_RING - 1)][lane];
#pragma unroll
			for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
			const int g = (int) ch.r0 + k;
			if (lane == 0) scores[(size_t) c * C + (u32) g] = v;
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
		AnBest* o = res + (size_t) blockIdx.y * n + c;
		o->score = best;
		o->n_tied = ntied;
		for (int q = 0; q < VDJX_ANNOT_TIED; q++) o->tied[q] = q < ntied ? tl[w][q] : -1;
	}
}

// one thread per contig: the chunks in index order; the call when S reaches min_score
__global__ void k_iso_merge(const AnBest* __restrict__ res, u32 n, u32 nchunks, int min_score, vdjx_annot_hit* __restrict__ hits) {
	const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= n) return;
	int best = -1, nt = 0, tied[VDJX_ANNOT_TIED];
	for (u32 k = 0; k < nchunks; k++) {
		const AnBest b = res[(size_t) k * n + c];
		if (b.score > best) { best = b.score; nt = 0; }
		if (b.score == best) {
			for (int z = 0; z < b.n_tied && z < VDJX_ANNOT_TIED; z++)
				if (nt + z < VDJX_ANNOT_TIED) tied[nt + z] = b.tied[z];
			nt += b.n_tied;
		}
	}
	vdjx_annot_hit* h = hits + c;
	h->score = best < 0 ? 0 : best;
	if (best < 0 || best < min_score) {
		h->gene = -1;
		for (int z = 0; z < VDJX_ANNOT_TIED; z++) h->tied[z] = -1;
		return;
	}
	h->gene = tied[0];
	h->n_tied = nt;
	for (int z = 0; z < VDJX_ANNOT_TIED; z++) h->tied[z] = z < nt ? tied[z] : -1;
}

__global__ __launch_bounds__(64) void k_iso_trace(const char* __restrict__ contigs, int len, int T, const uint8_t* __restrict__ cols,
                                                  const AnAlign* __restrict__ al, AnParams p, uint8_t* __restrict__ dirs,
                                                  vdjx_annot_hit* __restrict__ hits) {
	__shared__ short Hb[3][ISO_TSTRIDE], Fb[2][ISO_TSTRIDE], Eb[ISO_TSTRIDE];
	const AnAlign a = al[blockIdx.x];
	an_trace_pair(contigs + (size_t) a.contig * len + (len - T), T, cols + a.gat, a.g, p, dirs + a.dir, hits + a.contig, len - T, &Hb[0][0],
	              &Fb[0][0], Eb, ISO_TSTRIDE);
}

extern "C" int vdjx_constant_load(vdjx_ctx* c, const char* seqs, const uint64_t* off, size_t n) {
	if (!c || (n && (!seqs || !off))) { vdjx_set_error("vdjx_constant_load: NULL argument"); return VDJX_EINVAL; }
	if (n > ISO_MAX_RECORDS) { vdjx_set_error("vdjx_constant_load: %zu records (at most %u)", n, ISO_MAX_RECORDS); return VDJX_EINVAL; }
	for (size_t r = 0; r < n; r++) {
		if (off[r + 1] < off[r]) { vdjx_set_error("vdjx_constant_load: offsets of record %zu decrease", r); return VDJX_EINVAL; }
		const u64 L = off[r + 1] - off[r];
		if (L == 0 || L >= 2048) { vdjx_set_error("vdjx_constant_load: record %zu has %llu bases (1 .. 2047)", r, (unsigned long long) L); return VDJX_EINVAL; }
	}
	c->cs_loaded = false;
	c->cs_at.clear();
	c->cs_len.clear();
	std::vector<uint8_t> h;
	h.reserve((n ? off[n] - off[0] : 0) + n + 1);
	for (size_t r = 0; r < n; r++) {
		c->cs_at.push_back(h.size());
		c->cs_len.push_back((u32) (off[r + 1] - off[r]));
		h.push_back(AN_SEP);
		for (u64 x = off[r]; x < off[r + 1]; x++) h.push_back(an_gcode(seqs[x]));
	}
	c->cs_at.push_back(h.size());
	h.push_back(AN_SEP);
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (h.size() > c->cs_cols_cap) {
		if (c->d_cs_cols) HIP_TRY(hipFree(c->d_cs_cols));
		c->d_cs_cols = nullptr;
		c->cs_cols_cap = 0;
		HIP_TRY(hipMalloc(&c->d_cs_cols, h.size()));
		c->cs_cols_cap = h.size();
	}
	HIP_TRY(hipMemcpy(c->d_cs_cols, h.data(), h.size(), hipMemcpyHostToDevice));
	c->cs_loaded = true;
	return VDJX_OK;
}

static double iso_us_since(std::chrono::steady_clock::time_point t) {
	return (double) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t).count();
}

extern "C" int vdjx_isotype(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_isotype_params* prm, vdjx_annot_hit* out_c,
                            int32_t* out_scores) {
	if (!c || !prm || (n && (!contigs || !out_c))) { vdjx_set_error("vdjx_isotype: NULL argument"); return VDJX_EINVAL; }
	if (prm->match < 1 || prm->match > 15 || prm->mismatch < 0 || prm->mismatch > 31 || prm->gap_open < 0 || prm->gap_open > 31 ||
	    prm->gap_extend < 0 || prm->gap_extend > 31 || prm->min_score < 0 || prm->tail < 16 || prm->tail > 64) {
		vdjx_set_error("vdjx_isotype: parameters match=%d mismatch=%d gap_open=%d gap_extend=%d min_score=%d tail=%d (match 1..15, mismatch and "
		               "the gap costs 0..31, min_score >= 0, tail 16..64)", prm->match, prm->mismatch, prm->gap_open, prm->gap_extend,
		               prm->min_score, prm->tail);
		return VDJX_EINVAL;
	}
	if (!c->cs_loaded) { vdjx_set_error("vdjx_isotype: no constant set is loaded (call vdjx_constant_load first)"); return VDJX_ESTATE; }
	c->stats["iso_cells"] = 0;
	c->stats["iso_score_us"] = 0;
	c->stats["iso_trace_us"] = 0;
	if (n == 0) return VDJX_OK;
	if (len < 1 || len >= 4096) { vdjx_set_error("vdjx_isotype: len=%d (1 .. 4095)", len); return VDJX_EINVAL; }
	if (n >= (1ull << 20)) { vdjx_set_error("vdjx_isotype: %zu contigs (at most 2^20 - 1 per call)", n); return VDJX_EINVAL; }
	if (memchr(contigs, 0, n * (size_t) len)) { vdjx_set_error("vdjx_isotype: contigs of unequal length (a NUL inside the %zu x %d characters)", n, len); return VDJX_EINVAL; }
	const auto t0 = std::chrono::steady_clock::now();
	const AnParams p = {prm->match, prm->mismatch, prm->gap_open + prm->gap_extend, prm->gap_extend};
	const int T = std::min(prm->tail, len);
	const u32 C = (u32) c->cs_len.size();

	std::vector<IsoChunk> chunks;
	u64 cells = 0;
	for (u32 a = 0; a < C;) {
		u32 b = a + 1;
		while (b < C && c->cs_at[b + 1] - c->cs_at[a] + 1 <= ISO_CHUNK_COLS) b++;
		chunks.push_back({c->cs_at[a], (u32) (c->cs_at[b] - c->cs_at[a] + 1), a, b - a});
		a = b;
	}
	for (u32 x : c->cs_len) cells += (u64) x * (u64) T * (u64) n;
	const u32 nck = (u32) chunks.size();

	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	vdjx_work wk(c);
	char* d_ct;
	IsoChunk* d_ck;
	int* d_scores;
	AnBest* d_res;
	vdjx_annot_hit* d_hits;
	HIP_TRY(wk.alloc(&d_ct, n * (size_t) len));
	HIP_TRY(wk.alloc(&d_ck, nck));
	HIP_TRY(wk.alloc(&d_scores, n * (size_t) C));
	HIP_TRY(wk.alloc(&d_res, (size_t) nck * n));
	HIP_TRY(wk.alloc(&d_hits, n));
	HIP_TRY(hipMemcpyAsync(d_ct, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
	if (nck) HIP_TRY(hipMemcpyAsync(d_ck, chunks.data(), nck * sizeof(IsoChunk), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_hits, 0, n * sizeof(vdjx_annot_hit), st));
	{
		vdjx_prof_scope ps(c, "k_iso_score");
		if (nck)
			hipLaunchKernelGGL(k_iso_score, dim3((u32) ((n + ISO_WAVES - 1) / ISO_WAVES), nck), dim3(64 * ISO_WAVES), 0, st, (const char*) d_ct,
			                   (u32) n, len, T, (const uint8_t*) c->d_cs_cols, (const IsoChunk*) d_ck, C, p, d_scores, d_res);
		hipLaunchKernelGGL(k_iso_merge, dim3((u32) ((n + 255) / 256)), dim3(256), 0, st, (const AnBest*) d_res, (u32) n, nck, prm->min_score,
		                   d_hits);
	}
	std::vector<vdjx_annot_hit> hh(n);
	HIP_TRY(hipMemcpyAsync(hh.data(), d_hits, n * sizeof(vdjx_annot_hit), hipMemcpyDeviceToHost, st));
	if (out_scores && C) HIP_TRY(hipMemcpyAsync(out_scores, d_scores, n * (size_t) C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	const double us_score = iso_us_since(t0);
	const auto t1 = std::chrono::steady_clock::now();

	// phase 2: the primary hits with S > 0, in launches of at most ISO_DIR_BYTES direction bytes
	std::vector<AnAlign> al;
	for (size_t q = 0; q < n; q++) {
		const vdjx_annot_hit& h = hh[q];
		if (h.gene < 0 || h.score <= 0) continue;
		al.push_back({(u32) q, 0u, 0, c->cs_at[(size_t) h.gene], (int) c->cs_len[(size_t) h.gene]});
	}
	if (!al.empty()) {
		AnAlign* d_al;
		uint8_t* d_dir;
		HIP_TRY(wk.alloc(&d_al, al.size()));
		std::vector<size_t> at{0};
		u64 used = 0, peak = 0;
		for (size_t x = 0; x < al.size(); x++) {
			const u64 b = (u64) T * (u64) al[x].g;
			if (used && used + b > ISO_DIR_BYTES) { at.push_back(x); used = 0; }
			al[x].dir = used;
			used += b;
			peak = std::max(peak, used);
		}
		at.push_back(al.size());
		HIP_TRY(wk.alloc(&d_dir, peak));
		HIP_TRY(hipMemcpyAsync(d_al, al.data(), al.size() * sizeof(AnAlign), hipMemcpyHostToDevice, st));
		vdjx_prof_scope ps(c, "k_iso_trace");
		for (size_t L = 0; L + 1 < at.size(); L++)
			hipLaunchKernelGGL(k_iso_trace, dim3((u32) (at[L + 1] - at[L])), dim3(64), 0, st, (const char*) d_ct, len, T,
			                   (const uint8_t*) c->d_cs_cols, (const AnAlign*) d_al + at[L], p, d_dir, d_hits);
	}
	HIP_TRY(hipMemcpyAsync(out_c, d_hits, n * sizeof(vdjx_annot_hit), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	vdjx_prof_collect(c, false);
	c->stats["iso_cells"] = cells;
	c->stats["iso_score_us"] = (uint64_t) us_score;
	c->stats["iso_trace_us"] = (uint64_t) iso_us_since(t1);
	return VDJX_OK;
}
