// vdjx_vhit.h -- what every consumer of a caller-supplied V(D)J hit needs: vdjx_mutate.hip and vdjx_select.hip share it (gfx950 only, wave64).
//
// Device: a hit's runs become rows of a segment table in LDS, {first column, first contig index, first germline column, op | region << 2},
// and V's germline codons are resolved through V's 64 slots of it.
//   vh_aa, vh_ccode    the standard genetic code and the base code it is indexed by
//   vh_hit_segments    one lane per run of one hit: the lane's row from three wave-wide exclusive scans (columns, contig bases, germline
//                      bases) and the three totals.  A slot without a run is empty at its section's end and carries the totals, so the first
//                      columns (and, inside V, the germline columns) ascend over the table
//   vh_codon_range     the codons of the record that lie inside germ_start .. germ_end
//   vh_codon           a germline codon's three contig and germline codes; false where the codon cannot be classified
//   vh_subst_aa        the amino acid of a codon with one base replaced
// Host: the hits are the caller's, so every one of them is checked before anything reaches the device -- every index the kernels form lies
// inside the contig, the record and the row buffers because the run lengths were summed here.
//   vh_called, vh_usable, vh_run_sums, vh_check        one hit against its record set
//   vh_check_sizes, vh_check_contigs                   what a call checks of its contig block before it looks at a hit
// Everything here has internal linkage.
#pragma once
#include "vdjx_common.h"

#include <algorithm>
#include <string.h>

// the standard genetic code, codon 16 a + 4 b + c with A 0, C 1, G 2, T 3
__constant__ char vh_aa[65] = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";

__device__ __forceinline__ int vh_ccode(char ch) { return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4; }

// the lane's row of a hit's section: its nr runs start at runs[first], its first column is colbase, seq0 = seq_start - 1, at0 = the column of its
// base germ_start in its set's columns.  The hit loses its first `drop` columns (a clipped J): a run wholly inside them becomes empty, the
// run they end in is trimmed.  tc, tb, tg: the hit's columns (the dropped ones included), contig bases and germline bases
__device__ __forceinline__ int4 vh_hit_segments(const u32* __restrict__ runs, u32 first, int nr, u32 lane, int colbase, int seq0, int at0, int drop, int region,
                                                int& tc, int& tb, int& tg) {
	const bool live = (int) lane < nr;
	const u32 r = live ? runs[first + lane] : 0u;
	const int L = (int) (r >> 4), op = (int) (r & 15u);
	const int ec = vdjx_wave_excl(L, lane, tc), eb = vdjx_wave_excl(op != 2 ? L : 0, lane, tb), eg = vdjx_wave_excl(op != 1 ? L : 0, lane, tg);
	const int keep = max(0, min(L, ec + L - drop)), trim = L - keep;      // (a run wholly inside the dropped columns keeps nothing)
	int4 s = make_int4(colbase + max(ec - drop, 0), seq0 + eb + (op != 2 ? trim : 0), at0 + eg + (op != 1 ? trim : 0), op | region << 2);
	if (!live) s = make_int4(colbase + tc - drop, seq0 + tb, at0 + tg, s.w);
	return s;
}

// codons c_lo .. c_hi - 1 of the record: those wholly inside the vgerm germline bases that follow base v_germ0 (= germ_start - 1)
__device__ __forceinline__ void vh_codon_range(int v_germ0, int vgerm, int& c_lo, int& c_hi) {
	c_lo = (v_germ0 + 2) / 3;
	c_hi = (v_germ0 + vgerm) / 3;
}

// codon cd of V's record through V's slots seg[0 .. 63]: cb, gb = the contig's and the germline's codes of its three bases.  True where it can
// be classified: all three bases sit in M runs below the limit, in three consecutive columns, and all six codes are ACGT
__device__ __forceinline__ bool vh_codon(const int4* seg, const char* __restrict__ ct, const uint8_t* __restrict__ gcols, u32 v_at, int v_germ0,
                                         int limit, int cd, int cb[3], int gb[3]) {
	int colb[3];
	bool ok = true;
#pragma unroll
	for (int b = 0; b < 3; b++) {
		const int ga = (int) v_at + 3 * cd + b - v_germ0;      // the base's column in the germline set
		int lo = 0, hi = 64;             // the last V slot whose first germline column is <= ga (an I run shares the next run's)
		while (hi - lo > 1) {
			const int mid = (lo + hi) >> 1;
			if (seg[mid].z <= ga) lo = mid; else hi = mid;
		}
		const int4 s = seg[lo];
		const int off = ga - s.z;
		ok = ok && (s.w & 3) == 0;
		colb[b] = s.x + off;
		const int pos = s.y + off;
		ok = ok && pos < limit;
		cb[b] = ok ? vh_ccode(ct[pos]) : 4;      // (pos is inside the contig whenever the slot is an M run)
		gb[b] = gcols[ga];
		ok = ok && cb[b] < 4 && gb[b] < 4;
	}
	return ok && colb[1] == colb[0] + 1 && colb[2] == colb[1] + 1;
}

// the amino acid of codon gc (16 a + 4 b + c) with base b replaced by x; aa: the genetic code (a copy of vh_aa in LDS)
__device__ __forceinline__ char vh_subst_aa(const char* aa, int gc, int b, int x) {
	const int sh = 4 - 2 * b;
	return aa[(gc & ~(3 << sh)) | (x << sh)];
}

// ---- the host's side -------------------------------------------------------------------------------------------------------------------
static inline bool vh_called(const vdjx_annot_hit& h) { return h.gene >= 0 && h.score > 0; }
static inline bool vh_usable(const vdjx_annot_hit& h) { return vh_called(h) && h.n_runs <= VDJX_ANNOT_RUNS; }

// the runs of a usable hit: columns, contig bases (M + I), germline bases (M + D); false: an op outside 0..2 or a length of 0
static inline bool vh_run_sums(const vdjx_annot_hit& h, int64_t& ncol, int64_t& nseq, int64_t& ngerm) {
	ncol = nseq = ngerm = 0;
	for (int r = 0; r < h.n_runs; r++) {
		const u32 L = h.runs[r] >> 4, op = h.runs[r] & 15u;
		if (op > 2 || L == 0) return false;
		ncol += L;
		if (op != 2) nseq += L;
		if (op != 1) ngerm += L;
	}
	return true;
}

// a usable hit of contig i against class cls of its record set: *slot = its record's place among the class's records.  who: the call's
// name; what: "V", "D", "J"
static inline int vh_check(const char* who, const char* what, size_t i, const vdjx_annot_hit& h, const vdjx_recset& s, int cls, int len, size_t* slot_out) {
	const std::vector<u32>& rec = s.rec[cls];
	const size_t slot = std::lower_bound(rec.begin(), rec.end(), (u32) h.gene) - rec.begin();
	if (slot >= rec.size() || rec[slot] != (u32) h.gene) {
		vdjx_set_error("%s: contig %zu: the %s hit's gene %d is not a %s record of the loaded set", who, i, what, h.gene, what);
		return VDJX_EINVAL;
	}
	int64_t nc, ns, ng;
	if (h.n_runs < 0 || !vh_run_sums(h, nc, ns, ng)) {
		vdjx_set_error("%s: contig %zu: the %s hit has a run with an op outside 0..2 or a length of 0 (n_runs %d)", who, i, what, h.n_runs);
		return VDJX_EINVAL;
	}
	if (h.seq_start < 1 || h.germ_start < 1 || h.seq_end > len || (int64_t) h.germ_end > (int64_t) s.len[cls][slot]) {
		vdjx_set_error("%s: contig %zu: the %s hit's contig positions %d .. %d (1 .. %d) or germline positions %d .. %d (1 .. %u)", who, i, what,
		               h.seq_start, h.seq_end, len, h.germ_start, h.germ_end, s.len[cls][slot]);
		return VDJX_EINVAL;
	}
	if (ns != (int64_t) h.seq_end - h.seq_start + 1 || ng != (int64_t) h.germ_end - h.germ_start + 1) {
		vdjx_set_error("%s: contig %zu: the %s hit's runs hold %lld contig and %lld germline bases, its positions %d .. %d and %d .. %d", who, i, what,
		               (long long) ns, (long long) ng, h.seq_start, h.seq_end, h.germ_start, h.germ_end);
		return VDJX_EINVAL;
	}
	if (s.at[cls][slot] + (u64) s.len[cls][slot] >= (1ull << 31)) {
		vdjx_set_error("%s: contig %zu: the %s record lies past 2^31 columns of its set", who, i, what);
		return VDJX_EINVAL;
	}
	*slot_out = slot;
	return VDJX_OK;
}

// a call's contig block, in two steps so that a call's own argument checks can stand between them: the sizes ...
static inline int vh_check_sizes(const char* who, size_t n, int len) {
	if (len < 1 || len >= 4096) { vdjx_set_error("%s: len=%d (1 .. 4095)", who, len); return VDJX_EINVAL; }
	if (n >= (1ull << 20)) { vdjx_set_error("%s: %zu contigs (at most 2^20 - 1 per call)", who, n); return VDJX_EINVAL; }
	return VDJX_OK;
}
// ... and the characters, and the germline set they are laid against
static inline int vh_check_contigs(const char* who, const vdjx_ctx* c, const char* contigs, size_t n, int len) {
	if (memchr(contigs, 0, n * (size_t) len)) {
		vdjx_set_error("%s: contigs of unequal length (a NUL inside the %zu x %d characters)", who, n, len);
		return VDJX_EINVAL;
	}
	if (!c->germline.loaded) { vdjx_set_error("%s: no germline set is loaded (call vdjx_germline_load first)", who); return VDJX_ESTATE; }
	return VDJX_OK;
}
