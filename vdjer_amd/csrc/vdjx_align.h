// vdjx_align.h -- what the two local-alignment callers share (vdjx_annot.hip: contigs against V/J germlines; vdjx_iso.hip: contig tails
// against constant regions): the base codes, the reset column, the per-chunk result, and the traceback of one (query, record) pair.
// The model of both is in include/vdjx.h (vdjx_annotate).
#pragma once
#include "vdjx_common.h"

#define AN_SEP 6                         // the reset column's code
#define AN_NEG (-30000)                  // -inf of E and F (every real E, F is >= -62; every H is <= 15 * 2047)

struct AnParams { int ma, mi, oe, ext; };
struct AnBest { int score, n_tied, tied[VDJX_ANNOT_TIED]; };
struct AnAlign { u32 contig, cls; u64 dir; u64 gat; int g; };

__device__ __forceinline__ int an_ccode(char ch) {      // contig: A C G T -> 0..3, anything else 4
	return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
}
static inline uint8_t an_gcode(char ch) {               // germline: A C G T -> 0..3, anything else 5 (never equal to a contig's 4)
	return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 5;
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
