// vdjx_align.hip -- the local-alignment engine (affine gaps; the model is in include/vdjx.h, vdjx_annotate) and its three callers:
//   vdjx_germline_load / vdjx_annotate    whole contigs against the V and the J germlines (two classes, a call per class)
//   vdjx_constant_load / vdjx_isotype     the last T bases of every contig against the constant records (one class, every score kept)
//   vdjx_dsegment_load / vdjx_dcall       a window of each contig's own (start, length <= 256) against the D records (one class, every score kept)
// A query is a window of a contig (offset q0, m bases: one for all contigs, or -- the WIN forms of the kernels -- each contig's own, the
// launch sized to the longest).  Every query is scored against every record of a set, the best records of each
// class are kept, and the primary hit of each class is aligned again with direction bits and traced back.  Integer arithmetic
// throughout, no atomics on results: bitwise reproducible.
//
//   record set   per class the records' base codes back to back, each after a reset column, one more reset column at the end
//                (vdjx_recset).  A chunk is a run of consecutive records of a class (the caller's limits: columns, records).
//   phase 1      k_an_score: a wave per (contig, chunk), AN_WAVES contigs of one chunk per workgroup.  The query's rows are striped
//                over the lanes (lane l holds rows l*R+1 .. l*R+R in registers, H and E of the column before); the chunk's columns stream
//                through as a skewed systolic pipeline: at step t lane l computes column t - l and hands the (H, F) of its last row to
//                lane l + 1 (one shift per step).  A reset column clears a lane's rows, so records follow each other without a new fill.
//                When a lane passes the reset column after record k it parks its running maximum in its own slot of an LDS ring;
//                when lane 63 passes it, the whole wave reduces the slots: S of record k (written to the score matrix where the caller
//                keeps one), and the wave keeps the chunk's best S, how many records hold it and the first VDJX_ANNOT_TIED of them.
//                k_an_merge folds the chunks of a class in index order and makes the call.
//   phase 2      k_an_trace: a workgroup of one wave per primary hit recomputes the matrix by anti-diagonals (three H, two F and one E
//                diagonal in LDS, sized to the query or to the tail's bound), writes a direction byte per cell to the workspace (bits 0-1: where H came from
//                -- 0 stop, 1 diagonal, 2 E, 3 F; bit 2: E opened here; bit 3: F opened here), finds the first cell in row-major order
//                that holds S, and lane 0 walks the directions back; the coordinates come out in the contig's.
#include "vdjx_common.h"

#include <algorithm>
#include <string.h>

#define AN_SEP 6                         // the reset column's code
#define AN_NEG (-30000)                  // -inf of E and F (every real E, F is >= -62; every H is <= 15 * 2047)
#define AN_WAVES 4                       // contigs (waves) per workgroup of the scoring kernel, all over one chunk
#define AN_RING 32                       // records in flight per wave: each takes >= 2 columns, and a record is in flight 64 steps
#define AN_DIR_BYTES (256ull << 20)      // direction bytes per traceback launch
#define AN_TAIL_STRIDE 66                // shorts between the traceback's LDS diagonals for a query of at most 64 bases (rows 0 .. 64)
#define AN_CHUNK_COLS 65536u             // vdjx_annotate: columns per chunk at most
#define AN_PAIRS 16777216u               // vdjx_annotate: (contig, germline) pairs per scoring launch (VDJX_ANNOT_PAIRS)
#define ISO_CHUNK_COLS 2304u             // vdjx_isotype: columns per chunk at most (a record of 2047 bases and its two reset columns fit)
#define ISO_MAX_RECORDS 4096u
#define DC_CHUNK_COLS 2304u              // vdjx_dcall: columns per chunk at most (the widths tried)

struct AnParams { int ma, mi, oe, ext; };
struct AnChunk { u64 col0; u32 ncols, g0, ng; };
struct AnBest { int score, n_tied, tied[VDJX_ANNOT_TIED]; };
struct AnAlign { u32 contig, cls; u64 dir; u64 gat; int g; };

__device__ __forceinline__ int an_ccode(char ch) {      // contig: A C G T -> 0..3, anything else 4
	return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
}
static inline uint8_t an_gcode(char ch) {               // record: A C G T -> 0..3, anything else 5 (never equal to a contig's 4)
	return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 5;
}

// the query of contig c is queries[c * len .. + m) (the caller's pointer is at the window's offset in contig 0); MATRIX: scores[c * C + record] = S
// of every record as well.  WIN: the query of contig c is queries[c * len + win[c].x .. + win[c].y) instead, win[c].y <= 64 R (a row at or
// past the wave's own length holds the base that matches nothing, as the rows past m do); a wave without a query (win[c].y == 0) writes its
// zeros to the matrix and reports no record at all
template <int R, bool MATRIX, bool WIN = false>
__global__ __launch_bounds__(64 * AN_WAVES) void k_an_score(const char* __restrict__ queries, u32 n, u32 len, int m,
                                                           const uint8_t* __restrict__ cols, const AnChunk* __restrict__ chunks,
                                                           const u32* __restrict__ genes, const uint2* __restrict__ items, AnParams p, u32 C,
                                                           int* __restrict__ scores, AnBest* __restrict__ res,
                                                           const int2* __restrict__ win = nullptr) {
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
	if (WIN) {
		const int2 wn = win[c];
		queries += wn.x;
		m = wn.y;
	}
	int cb[R], H[R], E[R];
#pragma unroll
	for (int r = 0; r < R; r++) {
		const int i0 = (int) lane * R + r;                // rows past m compute too (a base that matches nothing): they can never hold more than a real row
		cb[r] = i0 < m ? an_ccode(queries[(size_t) c * len + i0]) : 7;
		H[r] = 0;
		E[r] = AN_NEG;
	}
	int cur = 0, seen = 0, best = -1, ntied = 0;
	int hin = 0, fin = AN_NEG, hdiag = 0;
	int bnext = -(int) lane >= 0 && -(int) lane < T ? cc[0] : AN_SEP;      // (step 0's column, by the loop's rule)
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
		if (__builtin_amdgcn_readlane(fl, 63)) {              // lane 63 has passed record k: every lane's maximum is parked
			const int k = __builtin_amdgcn_readlane(seen, 63) - 2;
			int v = ring[w][k & (AN_RING - 1)][lane];
#pragma unroll
			for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
			const int g = (int) gn[k];
			if (MATRIX && lane == 0) scores[(size_t) c * C + (u32) g] = v;
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
		if (WIN && m == 0) best = -1, ntied = 0;
		o->score = best;
		o->n_tied = ntied;
		for (int q = 0; q < VDJX_ANNOT_TIED; q++) o->tied[q] = q < ntied ? tl[w][q] : -1;
	}
}

// one thread per (class, contig): the chunks [ck.x, ck.y) of the class in index order; the call when S reaches the class's minimum
__global__ void k_an_merge(const AnBest* __restrict__ res, u32 n, u32 ncls, uint2 ck0, uint2 ck1, int min0, int min1,
                           vdjx_annot_hit* __restrict__ hits) {
	const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= ncls * n) return;
	const u32 cls = q >= n, c = q - cls * n;
	const uint2 ck = cls ? ck1 : ck0;
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
	vdjx_annot_hit* h = hits + q;
	h->score = best < 0 ? 0 : best;
	if (best < 0 || best < (cls ? min1 : min0)) {
		h->gene = -1;
		for (int z = 0; z < VDJX_ANNOT_TIED; z++) h->tied[z] = -1;
		return;
	}
	h->gene = tied[0];
	h->n_tied = nt;
	for (int z = 0; z < VDJX_ANNOT_TIED; z++) h->tied[z] = z < nt ? tied[z] : -1;
}

// One wave aligns the m query bases ct[0 .. m) with the record gc[1 .. g] (gc[0]: its reset column) again, by anti-diagonals (three H,
// two F and one E diagonal in LDS, `stride` shorts apart: stride > m), writes a direction byte per cell to dir[m * g] (bits 0-1: where H
// came from -- 0 stop, 1 diagonal, 2 E, 3 F; bit 2: E opened here; bit 3: F opened here), finds the first cell in row-major order that
// holds hit->score, and lane 0 walks the directions back into `hit`.  seq_start / seq_end come out `shift` higher (a query that is the
// tail of a longer sequence).  The workgroup is this one wave.
__device__ __forceinline__ void an_trace_pair(const char* __restrict__ ct, int m, const uint8_t* __restrict__ gc, int g, AnParams p,
                                              uint8_t* __restrict__ dir, vdjx_annot_hit* __restrict__ hit, int shift, short* Hb, short* Fb,
                                              short* Eb, int stride) {
	const u32 lane = threadIdx.x;
	const int S = hit->score;
	u32 cand = 0xFFFFFFFFu;
	for (int d = 2; d <= m + g; d++) {
		short* Hc = Hb + (d % 3) * stride;
		const short* H1 = Hb + ((d - 1) % 3) * stride;
		const short* H2 = Hb + ((d - 2) % 3) * stride;
		short* Fc = Fb + (d & 1) * stride;
		const short* F1 = Fb + ((d - 1) & 1) * stride;
		const int ilo = max(1, d - g), ihi = min(m, d - 1);
		for (int i = ilo + (int) lane; i <= ihi; i += 64) {
			const int j = d - i;
			const int diag = i > 1 && j > 1 ? H2[i - 1] : 0;
			const int hl = j > 1 ? H1[i] : 0, el = j > 1 ? Eb[i] : AN_NEG;
			const int hu = i > 1 ? H1[i - 1] : 0, fu = i > 1 ? F1[i - 1] : AN_NEG;
			const int s = an_ccode(ct[i - 1]) == gc[j] ? p.ma : -p.mi;
			const int eo = hl - p.oe, e = max(el - p.ext, eo);
			const int fo = hu - p.oe, f = max(fu - p.ext, fo);
			const int dg = diag + s;
			const int h = max(max(dg, 0), max(e, f));
			const int src = h == 0 ? 0 : h == dg ? 1 : h == e ? 2 : 3;
			const u32 at = (u32) (i - 1) * (u32) g + (u32) (j - 1);
			dir[at] = (uint8_t) (src | (e == eo ? 4 : 0) | (f == fo ? 8 : 0));
			Hc[i] = (short) h;
			Eb[i] = (short) max(e, AN_NEG);
			Fc[i] = (short) max(f, AN_NEG);
			if (h == S) cand = min(cand, at);
		}
		__syncthreads();
	}
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) cand = min(cand, (u32) __shfl_xor((int) cand, o, 64));
	if (lane != 0 || cand == 0xFFFFFFFFu) return;
	const int ie = (int) (cand / (u32) g) + 1, je = (int) (cand % (u32) g) + 1;
	int i = ie, j = je, st = 0, nm = 0, nx = 0, ni = 0, nd = 0, no = 0, nr = 0, lop = -1, llen = 0;
	for (;;) {
		int op;
		if (st == 0) {
			if (i == 0 || j == 0) break;
			const int dv = dir[(u32) (i - 1) * (u32) g + (u32) (j - 1)], src = dv & 3;
			if (src == 0) break;
			if (src == 2) { st = 1; continue; }
			if (src == 3) { st = 2; continue; }
			if (an_ccode(ct[i - 1]) == gc[j]) nm++; else nx++;
			op = 0;
			i--; j--;
		} else if (st == 1) {
			const int dv = dir[(u32) (i - 1) * (u32) g + (u32) (j - 1)];
			op = 2;
			nd++;
			if (dv & 4) { no++; st = 0; }
			j--;
		} else {
			const int dv = dir[(u32) (i - 1) * (u32) g + (u32) (j - 1)];
			op = 1;
			ni++;
			if (dv & 8) { no++; st = 0; }
			i--;
		}
		if (op == lop) { llen++; continue; }
		if (lop >= 0) { if (nr < VDJX_ANNOT_RUNS) hit->runs[nr] = (u32) llen << 4 | (u32) lop; nr++; }
		lop = op;
		llen = 1;
	}
	if (lop >= 0) { if (nr < VDJX_ANNOT_RUNS) hit->runs[nr] = (u32) llen << 4 | (u32) lop; nr++; }
	if (nr <= VDJX_ANNOT_RUNS) {
		for (int x = 0, y = nr - 1; x < y; x++, y--) { const u32 t = hit->runs[x]; hit->runs[x] = hit->runs[y]; hit->runs[y] = t; }
	} else {
		for (int x = 0; x < VDJX_ANNOT_RUNS; x++) hit->runs[x] = 0;
	}
	hit->seq_start = i + 1 + shift;
	hit->seq_end = ie + shift;
	hit->germ_start = j + 1;
	hit->germ_end = je;
	hit->matches = nm;
	hit->mismatches = nx;
	hit->ins = ni;
	hit->del = nd;
	hit->opens = no;
	hit->n_runs = nr;
}

// the launch's dynamic LDS holds the six diagonals, `stride` shorts apart: STRIDE where the caller's queries have a fixed bound (a tail:
// AN_TAIL_STRIDE, 792 bytes, and LDS addresses the compiler knows), else (STRIDE = 0) m + 1 for rows 0 .. m (48 KB at m = 4095).
// WIN: the alignment's query is its contig's own window win[contig] = (q0, m) of at most the launch's m bases (the LDS is sized to that).
template <int STRIDE, bool WIN = false>
__global__ __launch_bounds__(64) void k_an_trace(const char* __restrict__ contigs, int len, int q0, int m, const uint8_t* __restrict__ cols,
                                                 const AnAlign* __restrict__ al, AnParams p, uint8_t* __restrict__ dirs, u32 n,
                                                 vdjx_annot_hit* __restrict__ hits, const int2* __restrict__ win = nullptr) {
	extern __shared__ short diags[];
	const int stride = STRIDE ? STRIDE : m + 1;
	const AnAlign a = al[blockIdx.x];
	if (WIN) {
		const int2 wn = win[a.contig];
		q0 = wn.x;
		m = wn.y;
	}
	an_trace_pair(contigs + (size_t) a.contig * len + q0, m, cols + a.gat, a.g, p, dirs + a.dir, hits + (size_t) a.cls * n + a.contig, q0, diags,
	              diags + 3 * stride, diags + 5 * stride, stride);
}

// Builds the set from the records r with cls[r] >= 0 (their class; every such record has 1 .. 2047 bases) and uploads its columns.
static int an_set_load(vdjx_ctx* c, vdjx_recset& s, int ncls, const char* seqs, const uint64_t* off, const int8_t* cls, size_t n) {
	s.loaded = false;
	s.ncls = ncls;
	s.given = n;
	std::vector<uint8_t> h;
	for (int k = 0; k < ncls; k++) {
		s.rec[k].clear();
		s.at[k].clear();
		s.len[k].clear();
		for (size_t r = 0; r < n; r++) {
			if (cls[r] != k) continue;
			s.rec[k].push_back((u32) r);
			s.at[k].push_back(h.size());
			s.len[k].push_back((u32) (off[r + 1] - off[r]));
			h.push_back(AN_SEP);
			for (u64 x = off[r]; x < off[r + 1]; x++) h.push_back(an_gcode(seqs[x]));
		}
		s.at[k].push_back(h.size());
		h.push_back(AN_SEP);
	}
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	HIP_TRY(s.d_cols.reserve(h.size(), 0));
	HIP_TRY(hipMemcpy(s.d_cols, h.data(), h.size(), hipMemcpyHostToDevice));
	s.loaded = true;
	return VDJX_OK;
}

extern "C" int vdjx_germline_load(vdjx_ctx* c, const char* seqs, const uint64_t* off, const char* cls, size_t n) {
	if (!c || (n && (!seqs || !off || !cls))) { vdjx_set_error("vdjx_germline_load: NULL argument"); return VDJX_EINVAL; }
	if (n >= (1ull << 20)) { vdjx_set_error("vdjx_germline_load: %zu records (at most 2^20 - 1)", n); return VDJX_EINVAL; }
	std::vector<int8_t> k(n);
	for (size_t r = 0; r < n; r++) {
		k[r] = cls[r] == 'V' ? 0 : cls[r] == 'J' ? 1 : -1;
		if (off[r + 1] < off[r]) { vdjx_set_error("vdjx_germline_load: offsets of record %zu decrease", r); return VDJX_EINVAL; }
		const u64 L = off[r + 1] - off[r];
		if (k[r] >= 0 && (L == 0 || L >= 2048)) { vdjx_set_error("vdjx_germline_load: record %zu has %llu bases (1 .. 2047)", r, (unsigned long long) L); return VDJX_EINVAL; }
	}
	return an_set_load(c, c->germline, 2, seqs, off, k.data(), n);
}

extern "C" int vdjx_constant_load(vdjx_ctx* c, const char* seqs, const uint64_t* off, size_t n) {
	if (!c || (n && (!seqs || !off))) { vdjx_set_error("vdjx_constant_load: NULL argument"); return VDJX_EINVAL; }
	if (n > ISO_MAX_RECORDS) { vdjx_set_error("vdjx_constant_load: %zu records (at most %u)", n, ISO_MAX_RECORDS); return VDJX_EINVAL; }
	for (size_t r = 0; r < n; r++) {
		if (off[r + 1] < off[r]) { vdjx_set_error("vdjx_constant_load: offsets of record %zu decrease", r); return VDJX_EINVAL; }
		const u64 L = off[r + 1] - off[r];
		if (L == 0 || L >= 2048) { vdjx_set_error("vdjx_constant_load: record %zu has %llu bases (1 .. 2047)", r, (unsigned long long) L); return VDJX_EINVAL; }
	}
	const std::vector<int8_t> k(n, 0);
	return an_set_load(c, c->constant, 1, seqs, off, k.data(), n);
}

extern "C" int vdjx_dsegment_load(vdjx_ctx* c, const char* seqs, const uint64_t* off, size_t n) {
	if (!c || (n && (!seqs || !off))) { vdjx_set_error("vdjx_dsegment_load: NULL argument"); return VDJX_EINVAL; }
	if (n > ISO_MAX_RECORDS) { vdjx_set_error("vdjx_dsegment_load: %zu records (at most %u)", n, ISO_MAX_RECORDS); return VDJX_EINVAL; }
	for (size_t r = 0; r < n; r++) {
		if (off[r + 1] < off[r]) { vdjx_set_error("vdjx_dsegment_load: offsets of record %zu decrease", r); return VDJX_EINVAL; }
		const u64 L = off[r + 1] - off[r];
		if (L == 0 || L >= 2048) { vdjx_set_error("vdjx_dsegment_load: record %zu has %llu bases (1 .. 2047)", r, (unsigned long long) L); return VDJX_EINVAL; }
	}
	const std::vector<int8_t> k(n, 0);
	return an_set_load(c, c->dsegment, 1, seqs, off, k.data(), n);
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

// what a caller asks of an_run, and what it gets back for its stats
struct AnCall {
	const char* who;                     // the caller's name in messages
	const vdjx_recset* set;
	int tail;                            // the query: the last min(tail, len) bases of every contig (0: all of it)
	const int32_t *win_start, *win_len;  // or, when not NULL, each contig's own window [n] (inside the contig, at most 256 bases: the caller checked)
	int min_score[2];                    // per class: the smallest S that is a call
	u32 chunk_cols, chunk_recs;          // a chunk's columns and records at most
	u64 pairs;                           // (contig, record) pairs per scoring launch at most
	bool matrix;                         // keep S of every (contig, record): the set's one class, a query of at most 64 bases (256 with windows)
	int32_t* out_scores;                 // [n][records], or NULL
	const char *scope_score, *scope_trace;
	vdjx_annot_hit* out[2];              // per class: [n]
	u64 cells, us_score, us_trace;
	u64 chunks, score_launches, trace_launches;   // the call's chunks, its scoring launches that held work, its traceback launches
};

// The two phases for n contigs of `len` characters (the header comment).  Nothing is done for n == 0.
static int an_run(vdjx_ctx* c, const char* contigs, size_t n, int len, AnParams p, AnCall& a) {
	a.cells = a.us_score = a.us_trace = 0;              // (they stay 0 unless the call succeeds)
	a.chunks = a.score_launches = a.trace_launches = 0;
	if (n == 0) return VDJX_OK;
	if (len < 1 || len >= 4096) { vdjx_set_error("%s: len=%d (1 .. 4095)", a.who, len); return VDJX_EINVAL; }
	if (n >= (1ull << 20)) { vdjx_set_error("%s: %zu contigs (at most 2^20 - 1 per call)", a.who, n); return VDJX_EINVAL; }
	if (memchr(contigs, 0, n * (size_t) len)) { vdjx_set_error("%s: contigs of unequal length (a NUL inside the %zu x %d characters)", a.who, n, len); return VDJX_EINVAL; }
	const auto t0 = std::chrono::steady_clock::now();
	const vdjx_recset& s = *a.set;
	const bool win = a.win_len != nullptr;
	std::vector<int2> wins(win ? n : 0);
	u64 rows = 0;                                          // query bases of all contigs
	int wmax = 0;
	for (size_t q = 0; q < wins.size(); q++) {
		wins[q] = make_int2(a.win_start[q], a.win_len[q]);
		rows += (u64) a.win_len[q];
		wmax = std::max(wmax, a.win_len[q]);
	}
	const int ncls = s.ncls, m = win ? wmax : a.tail ? std::min(a.tail, len) : len, q0 = win ? 0 : len - m;
	if (!win) rows = (u64) m * (u64) n;

	// chunks: class by class; genes: the record index of every column run; items: chunk-major, AN_WAVES contigs each
	std::vector<AnChunk> chunks;
	std::vector<u32> genes;
	uint2 ck[2] = {};
	u64 cells = 0;
	for (int k = 0; k < ncls; k++) {
		ck[k].x = (u32) chunks.size();
		const u32 g0 = (u32) genes.size(), ng = (u32) s.rec[k].size();
		genes.insert(genes.end(), s.rec[k].begin(), s.rec[k].end());
		for (u32 x = 0; x < ng;) {
			u32 y = x + 1;
			while (y < ng && y - x < a.chunk_recs && s.at[k][y + 1] - s.at[k][x] + 1 <= a.chunk_cols) y++;
			chunks.push_back({s.at[k][x], (u32) (s.at[k][y] - s.at[k][x] + 1), g0 + x, y - x});
			x = y;
		}
		ck[k].y = (u32) chunks.size();
		for (u32 x : s.len[k]) cells += (u64) x * rows;
	}
	const u32 ngroups = (u32) ((n + AN_WAVES - 1) / AN_WAVES);
	std::vector<uint2> items;
	std::vector<u32> launch_at{0};
	u64 acc = 0;
	for (u32 q = 0; q < (u32) chunks.size(); q++)
		for (u32 gr = 0; gr < ngroups; gr++) {
			const u64 pp = (u64) std::min<u64>(AN_WAVES, n - (u64) gr * AN_WAVES) * chunks[q].ng;
			if (acc && acc + pp > a.pairs) { launch_at.push_back((u32) items.size()); acc = 0; }
			items.push_back(make_uint2(gr * AN_WAVES, q));
			acc += pp;
		}
	launch_at.push_back((u32) items.size());
	const size_t nck = chunks.size(), C = genes.size(), b_ck = nck * sizeof(AnChunk), b_it = items.size() * sizeof(uint2);
	std::vector<char> tab(b_ck + b_it + C * 4);           // chunks | items | genes: one upload
	if (C) {
		memcpy(tab.data(), chunks.data(), b_ck);
		memcpy(tab.data() + b_ck, items.data(), b_it);
		memcpy(tab.data() + b_ck + b_it, genes.data(), C * 4);
	}

	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	vdjx_work wk(c);
	char *d_ct, *d_tab;
	int2* d_win;
	int* d_scores;
	AnBest* d_res;
	vdjx_annot_hit* d_hits;
	HIP_TRY(wk.alloc(&d_ct, n * (size_t) len));
	HIP_TRY(wk.alloc(&d_tab, tab.size()));
	HIP_TRY(wk.alloc(&d_win, wins.size()));
	HIP_TRY(wk.alloc(&d_scores, a.matrix ? n * C : 0));
	HIP_TRY(wk.alloc(&d_res, nck * n));
	HIP_TRY(wk.alloc(&d_hits, ncls * n));
	HIP_TRY(hipMemcpyAsync(d_ct, contigs, n * (size_t) len, hipMemcpyHostToDevice, st));
	if (C) HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
	if (win) HIP_TRY(hipMemcpyAsync(d_win, wins.data(), wins.size() * sizeof(int2), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_hits, 0, ncls * n * sizeof(vdjx_annot_hit), st));
	const AnChunk* d_ck = (const AnChunk*) d_tab;
	const uint2* d_items = (const uint2*) (d_tab + b_ck);
	const u32* d_genes = (const u32*) (d_tab + b_ck + b_it);
	u64 score_launches = 0;
#define AN_LAUNCH(RR, MX, WN) hipLaunchKernelGGL((k_an_score<RR, MX, WN>), dim3(nb), dim3(64 * AN_WAVES), 0, st, (const char*) d_ct + q0, (u32) n, (u32) len, m, \
	(const uint8_t*) s.d_cols, d_ck, d_genes, d_items + b0, p, (u32) C, d_scores, d_res, (const int2*) d_win)
#define AN_CASE(RR) case RR: AN_LAUNCH(RR, false, false); break;
#define AN_CASE_WIN(RR) case RR: AN_LAUNCH(RR, true, true); break;
	{
		vdjx_prof_scope ps(c, a.scope_score);
		for (size_t L = 0; L + 1 < launch_at.size(); L++) {
			const u32 b0 = launch_at[L], nb = launch_at[L + 1] - b0;
			if (!nb) continue;
			score_launches++;
			if (win) switch (an_rows(m)) {                  // (m <= 256: 1 .. 4 rows per lane)
				AN_CASE_WIN(1) AN_CASE_WIN(2) AN_CASE_WIN(3) AN_CASE_WIN(4)
			}
			else if (a.matrix) AN_LAUNCH(1, true, false);
			else switch (an_rows(m)) {
				AN_CASE(1) AN_CASE(2) AN_CASE(3) AN_CASE(4) AN_CASE(6) AN_CASE(8) AN_CASE(12) AN_CASE(16) AN_CASE(24) AN_CASE(32) AN_CASE(48) AN_CASE(64)
			}
		}
		hipLaunchKernelGGL(k_an_merge, dim3((u32) ((ncls * n + 255) / 256)), dim3(256), 0, st, (const AnBest*) d_res, (u32) n, (u32) ncls, ck[0], ck[1],
		                   a.min_score[0], a.min_score[1], d_hits);
	}
#undef AN_CASE_WIN
#undef AN_CASE
#undef AN_LAUNCH
	std::vector<vdjx_annot_hit> hh(ncls * n);
	HIP_TRY(hipMemcpyAsync(hh.data(), d_hits, hh.size() * sizeof(vdjx_annot_hit), hipMemcpyDeviceToHost, st));
	if (a.out_scores && C) HIP_TRY(hipMemcpyAsync(a.out_scores, d_scores, n * C * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	const u64 us_score = (u64) an_us_since(t0);
	const auto t1 = std::chrono::steady_clock::now();

	// phase 2: the primary hits with S > 0, in launches of at most AN_DIR_BYTES direction bytes
	std::vector<AnAlign> al;
	std::vector<size_t> at{0};
	u64 used = 0, peak = 0;
	for (int k = 0; k < ncls; k++)
		for (size_t q = 0; q < n; q++) {
			const vdjx_annot_hit& h = hh[(size_t) k * n + q];
			if (h.gene < 0 || h.score <= 0) continue;
			const size_t slot = std::lower_bound(s.rec[k].begin(), s.rec[k].end(), (u32) h.gene) - s.rec[k].begin();
			const u64 b = (u64) (win ? a.win_len[q] : m) * s.len[k][slot];
			if (used && used + b > AN_DIR_BYTES) { at.push_back(al.size()); used = 0; }
			al.push_back({(u32) q, (u32) k, used, s.at[k][slot], (int) s.len[k][slot]});
			used += b;
			peak = std::max(peak, used);
		}
	if (!al.empty()) {
		AnAlign* d_al;
		uint8_t* d_dir;
		at.push_back(al.size());
		HIP_TRY(wk.alloc(&d_al, al.size()));
		HIP_TRY(wk.alloc(&d_dir, peak));
		HIP_TRY(hipMemcpyAsync(d_al, al.data(), al.size() * sizeof(AnAlign), hipMemcpyHostToDevice, st));
		vdjx_prof_scope ps(c, a.scope_trace);
		const bool fixed = a.matrix && !win;                // (a tail: at most 64 rows)
		const auto trace = win ? k_an_trace<0, true> : fixed ? k_an_trace<AN_TAIL_STRIDE> : k_an_trace<0>;
		const size_t lds = 6 * sizeof(short) * (fixed ? AN_TAIL_STRIDE : m + 1);
		for (size_t L = 0; L + 1 < at.size(); L++)
			hipLaunchKernelGGL(trace, dim3((u32) (at[L + 1] - at[L])), dim3(64), lds, st, (const char*) d_ct, len, q0, m, (const uint8_t*) s.d_cols,
			                   (const AnAlign*) d_al + at[L], p, d_dir, (u32) n, d_hits, (const int2*) d_win);
	}
	for (int k = 0; k < ncls; k++) HIP_TRY(hipMemcpyAsync(a.out[k], d_hits + (size_t) k * n, n * sizeof(vdjx_annot_hit), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipGetLastError());
	vdjx_prof_collect(c, false);
	a.cells = cells;
	a.us_score = us_score;
	a.us_trace = (u64) an_us_since(t1);
	a.chunks = nck;
	a.score_launches = score_launches;
	a.trace_launches = al.empty() ? 0 : at.size() - 1;
	return VDJX_OK;
}

static bool an_scores_ok(int ma, int mi, int go, int ge) { return ma >= 1 && ma <= 15 && mi >= 0 && mi <= 31 && go >= 0 && go <= 31 && ge >= 0 && ge <= 31; }

extern "C" int vdjx_annotate(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_annot_params* prm, vdjx_annot_hit* out_v,
                             vdjx_annot_hit* out_j) {
	if (!c || !prm || (n && (!contigs || !out_v || !out_j))) { vdjx_set_error("vdjx_annotate: NULL argument"); return VDJX_EINVAL; }
	if (!an_scores_ok(prm->match, prm->mismatch, prm->gap_open, prm->gap_extend)) {
		vdjx_set_error("vdjx_annotate: parameters match=%d mismatch=%d gap_open=%d gap_extend=%d (match 1..15, the others 0..31)", prm->match,
		               prm->mismatch, prm->gap_open, prm->gap_extend);
		return VDJX_EINVAL;
	}
	if (!c->germline.loaded) { vdjx_set_error("vdjx_annotate: no germline set is loaded (call vdjx_germline_load first)"); return VDJX_ESTATE; }
	static const u32 pairs = (u32) vdjx_env_num("VDJX_ANNOT_PAIRS", AN_PAIRS, 1, 0xFFFFFFFFll);
	AnCall a = {"vdjx_annotate", &c->germline, 0, nullptr, nullptr, {prm->min_v_score, prm->min_j_score}, AN_CHUNK_COLS, std::max<u32>(1u, pairs / AN_WAVES), pairs, false,
	            nullptr, "k_annot_score", "k_annot_trace", {out_v, out_j}};
	const int rc = an_run(c, contigs, n, len, {prm->match, prm->mismatch, prm->gap_open + prm->gap_extend, prm->gap_extend}, a);
	u64 trunc = 0;
	for (size_t q = 0; rc == VDJX_OK && q < n; q++) trunc += (out_v[q].n_runs > VDJX_ANNOT_RUNS) + (out_j[q].n_runs > VDJX_ANNOT_RUNS);
	c->stats["annot_cells"] = a.cells;
	c->stats["annot_score_us"] = a.us_score;
	c->stats["annot_trace_us"] = a.us_trace;
	c->stats["annot_chunks"] = a.chunks;
	c->stats["annot_score_launches"] = a.score_launches;
	c->stats["annot_trace_launches"] = a.trace_launches;
	c->stats["annot_cigar_truncated"] = trunc;
	return rc;
}

extern "C" int vdjx_isotype(vdjx_ctx* c, const char* contigs, size_t n, int len, const vdjx_isotype_params* prm, vdjx_annot_hit* out_c,
                            int32_t* out_scores) {
	if (!c || !prm || (n && (!contigs || !out_c))) { vdjx_set_error("vdjx_isotype: NULL argument"); return VDJX_EINVAL; }
	if (!an_scores_ok(prm->match, prm->mismatch, prm->gap_open, prm->gap_extend) || prm->min_score < 0 || prm->tail < 16 || prm->tail > 64) {
		vdjx_set_error("vdjx_isotype: parameters match=%d mismatch=%d gap_open=%d gap_extend=%d min_score=%d tail=%d (match 1..15, mismatch and "
		               "the gap costs 0..31, min_score >= 0, tail 16..64)", prm->match, prm->mismatch, prm->gap_open, prm->gap_extend,
		               prm->min_score, prm->tail);
		return VDJX_EINVAL;
	}
	if (!c->constant.loaded) { vdjx_set_error("vdjx_isotype: no constant set is loaded (call vdjx_constant_load first)"); return VDJX_ESTATE; }
	AnCall a = {"vdjx_isotype", &c->constant, prm->tail, nullptr, nullptr, {prm->min_score, 0}, ISO_CHUNK_COLS, ~0u, ~0ull, true, out_scores, "k_iso_score", "k_iso_trace",
	            {out_c, nullptr}};
	const int rc = an_run(c, contigs, n, len, {prm->match, prm->mismatch, prm->gap_open + prm->gap_extend, prm->gap_extend}, a);
	c->stats["iso_cells"] = a.cells;
	c->stats["iso_score_us"] = a.us_score;
	c->stats["iso_trace_us"] = a.us_trace;
	c->stats["iso_chunks"] = a.chunks;
	c->stats["iso_score_launches"] = a.score_launches;
	c->stats["iso_trace_launches"] = a.trace_launches;
	return rc;
}

extern "C" int vdjx_dcall(vdjx_ctx* c, const char* contigs, size_t n, int len, const int32_t* win_start, const int32_t* win_len,
                          const vdjx_dcall_params* prm, vdjx_annot_hit* out_d, int32_t* out_scores) {
	if (!c || !prm || (n && (!contigs || !win_start || !win_len || !out_d))) { vdjx_set_error("vdjx_dcall: NULL argument"); return VDJX_EINVAL; }
	if (!an_scores_ok(prm->match, prm->mismatch, prm->gap_open, prm->gap_extend) || prm->min_score < 0) {
		vdjx_set_error("vdjx_dcall: parameters match=%d mismatch=%d gap_open=%d gap_extend=%d min_score=%d (match 1..15, mismatch and the gap "
		               "costs 0..31, min_score >= 0)", prm->match, prm->mismatch, prm->gap_open, prm->gap_extend, prm->min_score);
		return VDJX_EINVAL;
	}
	if (!c->dsegment.loaded) { vdjx_set_error("vdjx_dcall: no D set is loaded (call vdjx_dsegment_load first)"); return VDJX_ESTATE; }
	for (size_t q = 0; q < n; q++)
		if (win_start[q] < 0 || win_len[q] < 0 || win_len[q] > VDJX_DCALL_WINDOW || (int64_t) win_start[q] + win_len[q] > len) {
			vdjx_set_error("vdjx_dcall: window %d + %d of contig %zu (start and length >= 0, at most %d bases, inside the %d bases of the contig)",
			               win_start[q], win_len[q], q, VDJX_DCALL_WINDOW, len);
			return VDJX_EINVAL;
		}
	AnCall a = {"vdjx_dcall", &c->dsegment, 0, win_start, win_len, {prm->min_score, 0}, DC_CHUNK_COLS, ~0u, ~0ull, true, out_scores, "k_dcall_score",
	            "k_dcall_trace", {out_d, nullptr}};
	const int rc = an_run(c, contigs, n, len, {prm->match, prm->mismatch, prm->gap_open + prm->gap_extend, prm->gap_extend}, a);
	c->stats["dcall_cells"] = a.cells;
	c->stats["dcall_score_us"] = a.us_score;
	c->stats["dcall_trace_us"] = a.us_trace;
	c->stats["dcall_chunks"] = a.chunks;
	c->stats["dcall_score_launches"] = a.score_launches;
	c->stats["dcall_trace_launches"] = a.trace_launches;
	return rc;
}
