/*
 * vdjer_main.c -- the `vdjer` command line (params.c:74-101, 214-298) over libvdjx (GPU hot path) and
 * vdjh (serial host stage).  Plain C; talks to the GPU only through the C ABI of include/vdjx.h.  The options: vdjer_cli.c (one
 * table; `vdjer --help` prints it); what a table flag does is said at its step below.
 *
 * Writes ./vdj_contigs.fa and ./vdjer.dot, SAM on stdout, log on stderr; exit 0 on success.
 *
 * --in: a BAM with its .bai (extraction as bam_read.c:264-446, restated over zlib in bamx.c), or -- recognised by its
 * content -- the extracted read pool as text, one read per line in extraction order:
 *     <pool:P|S> <name> <read_num:1|2> <is_rev:0|1> <SEQ> <QUAL>
 * from which the pool records (as-is + reverse complement, bam_read.c:206-244) are rebuilt.
 * stderr carries the reference's ELAPSED_SECS stage markers (status.c:22-32) in the reference's order; the k-mer table, prune and
 * graph build are ONE device call here, so the markers between PRE_PRE_GRAPH1 and POST_BUILD_GRAPH2 follow it back to back.
 */
#define _GNU_SOURCE
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>

#include "../../../include/vdjx.h"
#include "sph.h"
#include "vdjh.h"
#include "bamx.h"
#include "vdjx_mgpu.h"
#include "vdjx_newick.h"
#include "vdjer.h"
#include <errno.h>
#include <sys/wait.h>
#include <sys/resource.h>
#include <sys/prctl.h>
#include <signal.h>
#include <pthread.h>
#include <unistd.h>

typedef struct { int device; vdjx_ctx* gx; int rc; char err[512]; } init_job;
static void* init_thread(void* p) {
	init_job* j = (init_job*) p;
	j->rc = vdjx_init(j->device, &j->gx);
	if (j->rc) snprintf(j->err, sizeof j->err, "%s", vdjx_last_error());      /* (the message is the calling thread's) */
	return NULL;
}

static time_t t_start, t_prev;
static int g_rank;                             /* --gpus N: only rank 0 writes the stage log */
static int g_times;                            /* VDJX_TIMES (main reads it): more marks, each with its milliseconds */
static void status(const char* desc) {         /* status.c:22-32 without the /proc dumps */
	if (g_rank) return;
	if (g_times) {                 /* (diagnostic: milliseconds since the process started, beside the reference's whole seconds) */
		static struct timespec t0;
		struct timespec t;
		clock_gettime(CLOCK_MONOTONIC, &t);
		if (!t0.tv_sec) t0 = t;
		fprintf(stderr, "VDJX_TIMES\t%s\t%.1f\n", desc, (t.tv_sec - t0.tv_sec) * 1e3 + (t.tv_nsec - t0.tv_nsec) / 1e6);
	}
	time_t now = time(NULL);
	fprintf(stderr, "ELAPSED_SECS\t%s\t%ld\t%ld\n", desc, (long) (now - t_start), (long) (now - t_prev));
	t_prev = now;
}

/* ------------------------------------------------------------------------------------------ */
/* inputs                                                                                      */
/* ------------------------------------------------------------------------------------------ */
/* What one process holds of the read pool.  One GPU: all of it, the two pools as the reference lays them out (bam_read.c:376-379).
 * `--gpus N`: the process's SHARE -- the pairs whose read name hashes to its rank, both mates, all four records -- as ONE block
 * (`primary`: its primary-pool records followed by its secondary-pool ones, each group in extraction order), with every record's place
 * in the scan order of the whole pool and its registration rank over the whole pool beside it. */
typedef struct {
	int rl;
	uint8_t *primary, *secondary;
	size_t n_primary, n_secondary;      /* records */
	uint32_t *pair_id, *reg_rank;       /* per record of this process, block order */
	uint32_t* scan_index;               /* `--gpus N`: place in the whole pool's scan order (primary pool, then secondary) */
	uint8_t *read_num, *is_rc;
	char** names;                       /* by pair id (the process's own numbering); the characters live in `name_blocks` */
	void* name_blocks;
	uint32_t n_pairs;
	uint64_t total_records;             /* of the whole pool */
} reads_t;

static char comp(char c) { switch (c) { case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C'; default: return c; } }
static uint8_t comp_lut[256];
static void comp_init(void) { if (!comp_lut['A']) for (int i = 0; i < 256; i++) comp_lut[i] = (uint8_t) comp((char) i); }

/* one extracted read before it becomes two pool records */
typedef struct {
	char pool; char* name; int rn, rev; char* seq; char* qual;
	uint64_t seq_no, pool_no;           /* among all reads of the extraction / among the reads of its pool (kept by this process or not) */
} read_in;
typedef struct str_blk { struct str_blk* next; size_t used, cap; char data[]; } str_blk;
typedef struct {
	read_in* v; size_t n, cap;
	uint64_t np, ns;                    /* reads of the primary / secondary pool, kept or not */
	int max_len;
	int rank, nranks;
	int one_block;                      /* lay the records out as a share (one block), whatever nranks: the `--gpus N` code path */
	str_blk *strs, *name_strs;          /* sequences and qualities / names of the kept reads: appended to megabyte blocks (a malloc per field
	                                     * cost more than reading it); the names' blocks go on to the pool, which points into them */
} collector;

static char* blk_str(str_blk** head, const char* s, size_t n) {
	if (!*head || (*head)->used + n + 1 > (*head)->cap) {
		const size_t cap = n + 1 > ((size_t) 4 << 20) ? n + 1 : ((size_t) 4 << 20);
		str_blk* b = (str_blk*) malloc(sizeof(str_blk) + cap);
		if (!b) return NULL;
		b->next = *head; b->used = 0; b->cap = cap;
		*head = b;
	}
	char* p = (*head)->data + (*head)->used;
	memcpy(p, s, n);
	p[n] = 0;
	(*head)->used += n + 1;
	return p;
}
static char* col_str(collector* c, const char* s, size_t n) { return blk_str(&c->strs, s, n); }
static char* col_name(collector* c, const char* s, size_t n) { return blk_str(&c->name_strs, s, n); }

static uint64_t name_hash(const char* s) {
	uint64_t h = 1469598103934665603ull;
	for (; *s; s++) { h ^= (unsigned char) *s; h *= 1099511628211ull; }
	h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
	return h;
}
/* `--gpus N`: which rank owns the pair of this name */
static int owner_of(const char* name, int nranks) { return nranks > 1 ? (int) (name_hash(name) % (uint64_t) nranks) : 0; }
static int keep_name(void* ud, const char* name) { const collector* c = (const collector*) ud; return owner_of(name, c->nranks) == c->rank; }

/* (name must be NUL-terminated at name[ln]) */
static int collect_n(collector* c, char pool, const char* name, size_t ln, int rn, int rev, const char* seq, size_t ls, const char* qual, size_t lq) {
	const uint64_t seq_no = c->np + c->ns, pool_no = pool == 'P' ? c->np++ : c->ns++;
	const int l = (int) ls;
	if (l > c->max_len) c->max_len = l;                       /* get_read_length: the maximum (bam_read.c:264-292) */
	if (owner_of(name, c->nranks) != c->rank) return 0;
	if (c->n == c->cap) {
		c->cap = c->cap ? c->cap * 2 : 4096;
		c->v = (read_in*) realloc(c->v, c->cap * sizeof(read_in));
		if (!c->v) return -1;
	}
	read_in* x = &c->v[c->n++];
	x->pool = pool; x->rn = rn; x->rev = rev; x->seq_no = seq_no; x->pool_no = pool_no;
	x->name = col_name(c, name, ln); x->seq = col_str(c, seq, ls); x->qual = col_str(c, qual, lq);
	return x->name && x->seq && x->qual ? 0 : -1;
}
static void collector_free(collector* c) {
	for (str_blk* b = c->strs; b;) { str_blk* nx = b->next; free(b); b = nx; }
	for (str_blk* b = c->name_strs; b;) { str_blk* nx = b->next; free(b); b = nx; }
	free(c->v);
	memset(c, 0, sizeof *c);
}

/* add_to_buffer (bam_read.c:206-244) for every collected read: forward record, reverse-complement record, both registered.
 * One GPU: two pools, pair ids in extraction order.  A share: one block, primary-pool reads first. */
static int build_reads(const collector* c, reads_t* r) {
	const int rl = c->max_len, multi = c->one_block;
	size_t np = 0, ns = 0;
	for (size_t i = 0; i < c->n; i++) { if (c->v[i].pool == 'P') np++; else ns++; }
	memset(r, 0, sizeof *r);
	r->rl = rl;
	r->total_records = 2 * (c->np + c->ns);
	if (r->total_records >= (1ull << 32)) { fprintf(stderr, "more than 2^32 pool records\n"); return -1; }
	const size_t rec = 2 * (size_t) rl + 1;
	const size_t R = 2 * (np + ns);
	r->n_primary = multi ? R : 2 * np;
	r->n_secondary = multi ? 0 : 2 * ns;
	r->primary = (uint8_t*) calloc(r->n_primary * rec + 1, 1);
	r->secondary = multi ? NULL : (uint8_t*) calloc(r->n_secondary * rec + 1, 1);
	r->pair_id = (uint32_t*) calloc(R + 1, 4);
	r->reg_rank = (uint32_t*) calloc(R + 1, 4);
	r->scan_index = (uint32_t*) calloc(R + 1, 4);
	r->read_num = (uint8_t*) calloc(R + 1, 1);
	r->is_rc = (uint8_t*) calloc(R + 1, 1);
	r->names = (char**) calloc(np + ns + 1, sizeof(char*));
	if (!r->primary || (!multi && !r->secondary) || !r->pair_id || !r->reg_rank || !r->scan_index || !r->read_num || !r->is_rc || !r->names) { fprintf(stderr, "out of memory\n"); return -1; }
	sph_table ids;                       /* read name -> pair id */
	sph_init(&ids, 0, 0);
	comp_init();
	size_t ip = 0, is = 0;
	for (size_t q = 0; q < c->n; q++) {
		const read_in* in = &c->v[q];
		if ((int) strlen(in->seq) != rl || (int) strlen(in->qual) != rl) { fprintf(stderr, "read %s: length != %d\n", in->name, rl); sph_free(&ids); return -1; }
		size_t b = sph_find(&ids, in->name);
		uint32_t pid;
		if (b == (size_t) -1) {
			pid = r->n_pairs++;
			r->names[pid] = in->name;                          /* (in the collector's string blocks, which this pool takes over) */
			sph_map_put(&ids, r->names[pid], (void*) (uintptr_t) (pid + 1), NULL);
		} else {
			pid = (uint32_t) (uintptr_t) ids.b[b].val - 1;
		}
		const int isp = in->pool == 'P';
		const size_t g = isp ? ip : 2 * np + is;                /* first record of the read in this process's block order */
		uint8_t* base = multi || isp ? r->primary + g * rec : r->secondary + is * rec;
		base[0] = '0';
		memcpy(base + 1, in->seq, (size_t) rl);
		memcpy(base + 1 + rl, in->qual, (size_t) rl);
		base[rec] = '0';
		for (int i = 0; i < rl; i++) {
			base[rec + 1 + i] = comp_lut[(uint8_t) in->seq[rl - 1 - i]];
			base[rec + 1 + rl + i] = (uint8_t) in->qual[rl - 1 - i];
		}
		for (int j = 0; j < 2; j++) {
			r->pair_id[g + j] = pid;
			r->read_num[g + j] = (uint8_t) in->rn;
			r->is_rc[g + j] = (uint8_t) (j ? !in->rev : (in->rev != 0));     /* add_read_info(..., bam_is_rev) then (!bam_is_rev) */
			r->reg_rank[g + j] = (uint32_t) (2 * in->seq_no + (uint64_t) j);
			r->scan_index[g + j] = (uint32_t) ((isp ? 0 : 2 * c->np) + 2 * in->pool_no + (uint64_t) j);
		}
		if (isp) ip += 2; else is += 2;
	}
	sph_free(&ids);
	return 0;
}

/* --in <bam>: get_read_length + extract (bam_read.c:264-446) through bamx; a rank of `--gpus N` runs the same passes and keeps its share */
static int load_bam(const cli* c, collector* col) {
	if (!c->vdj_fasta[0] || !c->v_region[0] || !c->c_region[0]) { fprintf(stderr, "BAM input needs --chain/--ref-dir (or --vdjf, --vr, --cr)\n"); return -1; }
	bamx_reads br;
	bamx_threads(c->threads);                              /* (--t: blocks are inflated ahead of the parser in the sequential passes) */
	if (bamx_extract_filtered(c->in, c->vdj_fasta, c->v_region, c->c_region, col->nranks > 1 ? keep_name : NULL, col, &br)) { fprintf(stderr, "%s\n", bamx_last_error()); return -1; }
	if (br.read_len != br.max_len) {
		fprintf(stderr, "reads of different lengths (%d and %d): the reference lays its pools out with one length\n", br.read_len, br.max_len);
		bamx_free(&br);
		return -1;
	}
	col->v = (read_in*) calloc(br.n + 1, sizeof(read_in));
	col->cap = br.n + 1;
	for (size_t i = 0; i < br.n; i++) {
		const bamx_read* x = &br.v[i];
		read_in* o = &col->v[col->n++];
		o->pool = x->pool; o->rn = x->read_num; o->rev = x->is_rev; o->seq_no = x->seq_no; o->pool_no = x->pool_no;
		o->name = col_name(col, x->name, strlen(x->name));
		o->seq = col_str(col, x->seq, (size_t) br.read_len);         /* (read_len characters, NUL padded by the extraction if the record was shorter) */
		o->qual = col_str(col, x->qual, (size_t) br.read_len);
	}
	col->np = br.n_primary_reads; col->ns = br.n_secondary_reads;
	col->max_len = br.max_len;
	bamx_free(&br);
	return 0;
}

/* the extracted read pool as text (see the head of this file): every process reads the whole file once and keeps its share.
 * Six whitespace-separated fields per read (fscanf's "%s %s %d %d %s %s": any run of blanks or newlines separates), a few MB at a time. */
static int is_ws(char ch) { return ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r' || ch == '\f' || ch == '\v'; }
static int load_text(const char* path, collector* col) {
	FILE* fp = fopen(path, "r");
	const size_t CH = (size_t) 8 << 20;
	char* buf = (char*) malloc(CH + 1);
	if (!fp || !buf) { fprintf(stderr, "cannot open %s\n", path); if (fp) fclose(fp); free(buf); return -1; }
	size_t have = 0;
	int rc = 0, eof = 0, stop = 0;
	while (!stop && !rc) {
		if (!eof) {
			const size_t got = fread(buf + have, 1, CH - have, fp);
			have += got;
			if (got == 0) eof = 1;
		}
		buf[have] = 0;
		/* whole reads only: up to the last whitespace that ends a sixth field (at the end of the file: everything) */
		size_t at = 0;
		for (;;) {
			char* f[6];
			size_t fl[6];
			size_t p = at;
			int k = 0;
			for (; k < 6; k++) {
				while (p < have && is_ws(buf[p])) p++;
				if (p >= have) break;
				const size_t a0 = p;
				while (p < have && !is_ws(buf[p])) p++;
				if (p >= have && !eof) break;                       /* (the field may go on in the next piece) */
				f[k] = buf + a0; fl[k] = p - a0;
			}
			if (k < 6) { if (eof) stop = 1; break; }
			/* numbers as fscanf's %d reads them; a malformed line ends the input there, like the reference's format string would */
			char *e1, *e2;
			const char c2 = f[2][fl[2]], c3 = f[3][fl[3]];
			f[2][fl[2]] = 0; f[3][fl[3]] = 0;
			const long rn = strtol(f[2], &e1, 10), rv = strtol(f[3], &e2, 10);
			const int bad = *e1 || *e2 || fl[0] > 7 || fl[1] > 511 || fl[4] > 1023 || fl[5] > 1023;
			f[2][fl[2]] = c2; f[3][fl[3]] = c3;
			if (bad) { stop = 1; break; }
			f[1][fl[1]] = 0;                                        /* (the separator after the name: the name is hashed as a C string) */
			if ((rc = collect_n(col, f[0][0] == 'P' ? 'P' : 'S', f[1], fl[1], (int) rn, (int) rv, f[4], fl[4], f[5], fl[5])) != 0) { fprintf(stderr, "out of memory\n"); break; }
			at = p;
		}
		if (eof) break;
		memmove(buf, buf + at, have - at);
		have -= at;
		if (have == CH) { fprintf(stderr, "%s: a read of more than %zu bytes\n", path, CH); rc = -1; }
	}
	fclose(fp);
	free(buf);
	return rc;
}

static int load_reads(const cli* c, reads_t* r, int rank, int nranks, int as_share) {
	const int isbam = bamx_is_bam(c->in);
	if (isbam < 0) { fprintf(stderr, "cannot open %s\n", c->in); return -1; }
	collector col;
	memset(&col, 0, sizeof col);
	col.rank = rank; col.nranks = nranks; col.max_len = -1; col.one_block = as_share;
	int rc = isbam ? load_bam(c, &col) : load_text(c->in, &col);
	if (!rc && col.max_len <= 0) { fprintf(stderr, "Error retrieving read length from: %s\n", c->in); rc = -1; }
	if (!rc) rc = build_reads(&col, r);
	if (!rc) { r->name_blocks = col.name_strs; col.name_strs = NULL; }      /* (the names point into them) */
	collector_free(&col);
	return rc;
}

/* load_kmers, vj_filter.c:56-68 */
static int load_codes(const char* path, int max_dist, uint32_t** out, size_t* n) {
	FILE* in = fopen(path, "r");
	if (!in) { fprintf(stderr, "cannot open %s\n", path); return -1; }
	size_t cap = 1024, cnt = 0;
	uint32_t* v = (uint32_t*) malloc(cap * 4);
	unsigned long kmer;
	int freq;
	while (fscanf(in, "%lu\t%d\n", &kmer, &freq) == 2) {
		if (freq <= max_dist) {
			if (cnt == cap) { cap *= 2; v = (uint32_t*) realloc(v, cap * 4); }
			v[cnt++] = (uint32_t) kmer;
		}
	}
	fclose(in);
	*out = v;
	*n = cnt;
	return 0;
}

static int cmp_u32(const void* a, const void* b) { uint32_t x = *(const uint32_t*) a, y = *(const uint32_t*) b; return x < y ? -1 : x > y; }

/* score_seq_init's reader (seq_score.c:50-70): fgets chunks of 999,999 chars, header lines skipped */
static int load_vregion(const char* path, char*** lines, size_t* n) {
	FILE* fp = fopen(path, "r");
	if (!fp) { fprintf(stderr, "cannot open %s\n", path); return -1; }
	char* buf = (char*) malloc(1000000);
	size_t cap = 4, cnt = 0;
	char** v = (char**) malloc(cap * sizeof(char*));
	while (fgets(buf, 1000000, fp) != NULL) {
		if (buf[0] == '>') continue;
		size_t l = strlen(buf);
		if (l) buf[l - 1] = '\0';                        /* "Get rid of newline" */
		if (cnt == cap) { cap *= 2; v = (char**) realloc(v, cap * sizeof(char*)); }
		v[cnt++] = strdup(buf);
	}
	fclose(fp);
	free(buf);
	*lines = v;
	*n = cnt;
	return 0;
}

/* ------------------------------------------------------------------------------------------ */
/* hooks onto libvdjx                                                                          */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
	vdjx_ctx* gx; vdjx_mgpu* mg;
	const cli* c;                       /* the options */
	int tables_ran;                     /* the SAM body hook ran and tables() ended well (it is called at most once: only when there is a contig) */
	vdjx_quant_info qi;
	double* qcnt;                       /* --quant: its counts (the --airr table's expected_count) */
	double* qboot;                      /* --quant-boot: its qb_b x n replicate counts, replicate-major (the --lineages table's clone_count_sd) */
	vdjx_quant_boot_info qbi;
	size_t a_contigs, a_v, a_j, a_prod, a_trunc, a_skip_d, a_skip_other;
	struct germ_set* dset; vdjx_annot_hit* hd;          /* --d-calls: the D set (the class-D records of the germline FASTA) and the D hits (dcall_run) */
	size_t d_contigs, d_windows, d_over, d_called;
	/* --isotypes / --clones: what the steps above and vdjx_isotype found is kept until the last table is written */
	struct germ_set* germ; vdjx_annot_hit *hv, *hj;      /* the germline records and the V / J hits (annot_run) */
	struct germ_set* cst; vdjx_annot_hit* hc;            /* the constant records and the isotype hits (iso_run) */
	size_t i_contigs, i_called, c_rows, c_clusters;
	/* --lineages: the clone of every contig (lineage_run; -1: not eligible), kept for the --airr table's clone_id */
	int lin_num;                        /* the threshold's numerator: --lineage-dist's, until --lineage-threshold finds its own */
	unsigned long long lin_walked;      /* --lineage-model: the pairs walked */
	int32_t* lin_clone; vdjx_lineage_info li;
	vdjx_lineage_link_info lki;         /* --lineage-link: what vdjx_lineage_link reports */
	vdjx_threshold_info thi; int thr_fallback, thr_passes;    /* --lineage-threshold: what was found, the --lineage-dist numerator it stands in for, the pair passes made */
	size_t l_contigs, l_eligible;
	vdjx_tree_info ti;                  /* --trees (tree_run, after lineage_run) */
	vdjx_tree_nj_info tni;              /* --trees-nj (tree_nj_run, after tree_run) */
	vdjx_tree_mp_info tmi;              /* --trees-mp (tree_mp_run, after tree_nj_run) */
	vdjx_tree_support_info tsi;         /* --tree-support (tree_run) */
	/* --mutations: the germline rows of every contig (mut_run), kept for the --airr table's two alignment cells */
	uint64_t* mu_off; char *mu_seq, *mu_germ; vdjx_mut_info mi;
	/* --diversity: the Hill curve of the lineages (diversity_run, after lineage_run) */
	uint32_t dv_depth;                  /* --diversity-depth's, or (0) the total expected pairs once they are known */
	vdjx_diversity_info dvi; uint64_t dv_weight; double dv_d0, dv_d1, dv_d2;
	/* --selection: the selection strength of the V mutations (sel_run, after lineage_run) */
	vdjx_sel_info si; double sel_sigma[2]; size_t sel_unmatched;
	vdjx_selconv_info sci; double sel_msigma[2];      /* --selection-combine mean */
	/* --targeting-model: the sample's own targeting model (tgt_run, after lineage_run) */
	vdjx_tgt_info tgi; unsigned tgt_levels[2][4];      /* [substitution, mutability][level 5, 3, 1, 0]: the 5-mers on it */
	/* --consensus: the consensus of every lineage (cons_run, after lineage_run); the pseudo-contigs, their hits and first voters are kept for sel_run */
	vdjx_cons_info ci; uint32_t cs_largest;
	size_t cs_units; int cs_plen; char* cs_pc; vdjx_annot_hit* cs_hv; vdjx_cons_unit* cs_un; size_t* cs_first;
} hook_ud;


static int h_root_score(void* ud, const char* kmers, size_t n, int k, int thr, uint8_t* out) {
	hook_ud* u = (hook_ud*) ud;
	int rc = vdjx_root_score(u->gx, kmers, n, k, thr, out);
	if (rc) fprintf(stderr, "vdjx_root_score: %s\n", vdjx_last_error());
	return rc;
}

static int h_window_score(void* ud, const char* windows, size_t n, int len, uint8_t* valid) {
	hook_ud* u = (hook_ud*) ud;
	const vdjh_params* p = &u->c->hp;
	vdjx_cov_params cp = {p->eval_start, p->eval_stop, p->filter_read_span, p->filter_mate_span, p->insert_len, p->insert_len, p->read_filter_floor};
	if (u->mg) {                              /* `--gpus N`: every rank maps the windows against its share of the pool */
		const int rcm = vdjx_mgpu_window_score(u->mg, u->gx, windows, n, len, &cp, valid);
		if (rcm) fprintf(stderr, "vdjx_mgpu_window_score: %s\n", vdjx_mgpu_last_error());
		return rcm;
	}
	uint32_t* np = (uint32_t*) malloc((n + 1) * 4);
	int rc = vdjx_window_score(u->gx, windows, n, len, &cp, valid, np);
	if (rc) fprintf(stderr, "vdjx_window_score: %s\n", vdjx_last_error());
	free(np);
	return rc;
}

/* output_mapping, quick_map3.c:152-181: mapped and formatted on the device (vdjx_sam_text) */
static int sam_records(void* ud, const char* const* ids, const char* contigs, size_t n, int len, FILE* out) {
	hook_ud* u = (hook_ud*) ud;
	uint32_t* id_off = (uint32_t*) calloc(n + 1, 4);
	size_t tot = 0;
	for (size_t c = 0; c < n; c++) { tot += strlen(ids[c]); id_off[c + 1] = (uint32_t) tot; }
	char* cat = (char*) malloc(tot + 1);
	for (size_t c = 0; c < n; c++) memcpy(cat + id_off[c], ids[c], id_off[c + 1] - id_off[c]);
	const char* text = NULL;
	uint64_t nb = 0;
	int rc = u->mg ? vdjx_mgpu_sam_body(u->mg, u->gx, contigs, n, len, cat, id_off, &text, &nb) : vdjx_sam_text(u->gx, contigs, n, len, cat, id_off, &text, &nb);
	free(cat);
	free(id_off);
	if (rc) { fprintf(stderr, "%s: %s\n", u->mg ? "vdjx_mgpu_sam_body" : "vdjx_sam_text", u->mg ? vdjx_mgpu_last_error() : vdjx_last_error()); return rc; }
	if (nb && fwrite(text, 1, (size_t) nb, out) != (size_t) nb) { fprintf(stderr, "short write of the SAM records\n"); return -1; }
	return 0;
}

/* --quant: rsem-calculate-expression's <prefix>.isoforms.results (demo/quant_demo.bash) for the final contigs, in vdj_contigs.fa order:
 * every contig is its own gene, all have length `len`; TPM = 1e6 N / sum N, FPKM = 1e9 N / (eff_len sum N), IsoPct 100 or 0 */
static int quant_table(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) {
	double* cnt = (double*) calloc(n + 1, sizeof(double));
	const vdjx_quant_params qp = {10000, 1e-5};
	const uint32_t B = u->c->quant ? u->c->qb_b : 0;
	double* st = NULL;                  /* the bootstrap's summary: mean, sd, lower, upper, n each */
	int rc;
	if (B) {
		const vdjx_quant_boot_params bp = {(int) B, u->c->qb_seed};
		uint32_t* iters = (uint32_t*) calloc(B, sizeof(uint32_t));
		free(u->qboot);
		u->qboot = (double*) calloc((size_t) B * n + 1, sizeof(double));
		st = (double*) calloc(4 * n + 1, sizeof(double));
		rc = vdjx_quant_boot(u->gx, contigs, n, len, &qp, &bp, cnt, &u->qi, u->qboot, iters, &u->qbi);
		free(iters);
		if (!rc) vdjx_quant_boot_summary(u->qboot, B, n, st, st + n, st + 2 * n, st + 3 * n);
	} else rc = vdjx_quant(u->gx, contigs, n, len, &qp, cnt, &u->qi);
	if (rc) { fprintf(stderr, "%s: %s\n", B ? "vdjx_quant_boot" : "vdjx_quant", vdjx_last_error()); free(cnt); free(st); return rc; }
	if (!u->c->quant) { free(u->qcnt); u->qcnt = cnt; return 0; }      /* (--clones alone: the counts, no table) */
	FILE* fp = fopen(u->c->quant, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->quant); free(cnt); free(st); return -1; }
	free(u->qcnt);
	double sum = 0.0;
	for (size_t i = 0; i < n; i++) sum += cnt[i];
	const double eff = u->qi.eff_len;
	fprintf(fp, "transcript_id\tgene_id\tlength\teffective_length\texpected_count\tTPM\tFPKM\tIsoPct%s\n", B ? "\tboot_mean\tboot_sd\tboot_lower\tboot_upper" : "");
	for (size_t i = 0; i < n; i++) {
		const double tpm = sum > 0.0 ? 1e6 * cnt[i] / sum : 0.0, fpkm = sum > 0.0 && eff > 0.0 ? cnt[i] * 1e9 / (eff * sum) : 0.0;
		fprintf(fp, "%s\t%s\t%d\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f", ids[i], ids[i], len, eff, cnt[i], tpm, fpkm, cnt[i] > 0.0 ? 100.0 : 0.0);
		if (B) fprintf(fp, "\t%.2f\t%.2f\t%.2f\t%.2f", st[i], st[n + i], st[2 * n + i], st[3 * n + i]);
		fputc('\n', fp);
	}
	free(st);
	u->qcnt = cnt;
	if (fclose(fp)) { fprintf(stderr, "cannot write %s\n", u->c->quant); return -1; }
	return 0;
}

/* ---- --airr: the germline FASTA, the junction-derived fields and the table (the model: include/vdjx.h, vdjx_annotate) ---------------- */
typedef struct germ_set { char* seqs; uint64_t* off; char* cls; char** names; size_t n, cap, bytes, bcap; } germ_set;

/* the record's name: the header's first token, or its second '|' field when the token has one; its class: the 4th character of
 * IG[HKL]* / TR[ABDG]* names, the 1st otherwise */
static void germ_name(const char* head, char** name, char* cls) {
	size_t a = 0;
	while (head[a] && isspace((unsigned char) head[a])) a++;
	size_t b = a;
	while (head[b] && !isspace((unsigned char) head[b])) b++;
	const char* t = head + a;
	size_t tl = b - a;
	const char* bar = memchr(t, '|', tl);
	if (bar) {
		const char* s2 = bar + 1;
		const char* e2 = memchr(s2, '|', (size_t) (t + tl - s2));
		tl = (size_t) ((e2 ? e2 : t + tl) - s2);
		t = s2;
	}
	*name = strndup(t, tl);
	const char* nm = *name;
	const int imgt = tl >= 4 && ((nm[0] == 'I' && nm[1] == 'G' && strchr("HKL", nm[2])) || (nm[0] == 'T' && nm[1] == 'R' && strchr("ABDG", nm[2])));
	*cls = imgt ? nm[3] : tl ? nm[0] : '?';
}

static int germ_read(const char* path, germ_set* g, const char* what) {
	memset(g, 0, sizeof *g);
	FILE* fp = fopen(path, "r");
	if (!fp) { fprintf(stderr, "%s %s\n", what, path); return -1; }
	char* line = NULL;
	size_t lcap = 0;
	ssize_t ln;
	while ((ln = getline(&line, &lcap, fp)) >= 0) {
		if (line[0] == '>') {
			if (g->n + 2 > g->cap) {
				g->cap = g->cap ? 2 * g->cap : 256;
				g->off = (uint64_t*) realloc(g->off, (g->cap + 1) * sizeof(uint64_t));
				g->cls = (char*) realloc(g->cls, g->cap);
				g->names = (char**) realloc(g->names, g->cap * sizeof(char*));
			}
			g->off[g->n] = g->bytes;
			germ_name(line + 1, &g->names[g->n], &g->cls[g->n]);
			g->n++;
			continue;
		}
		if (!g->n) continue;
		for (ssize_t k = 0; k < ln; k++) {
			const unsigned char ch = (unsigned char) line[k];
			if (ch == '.' || isspace(ch)) continue;
			if (g->bytes + 1 > g->bcap) { g->bcap = g->bcap ? 2 * g->bcap : 65536; g->seqs = (char*) realloc(g->seqs, g->bcap); }
			g->seqs[g->bytes++] = (char) toupper(ch);
		}
	}
	free(line);
	fclose(fp);
	if (!g->off) g->off = (uint64_t*) calloc(1, sizeof(uint64_t));
	g->off[g->n] = g->bytes;
	if (!g->seqs) g->seqs = (char*) calloc(1, 1);
	return 0;
}

static char codon_aa(const char* c) {
	static const char* B = "TCAG";
	static const char* AA = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
	int v = 0;
	for (int k = 0; k < 3; k++) {
		const char* q = strchr(B, c[k]);
		if (!c[k] || !q) return 'X';
		v = 4 * v + (int) (q - B);
	}
	return AA[v];
}

static void put_aa(FILE* fp, const char* s, size_t n) { for (size_t q = 0; q + 3 <= n; q += 3) fputc(codon_aa(s + q), fp); }

static void put_call(FILE* fp, const vdjx_annot_hit* h, const germ_set* g) {
	if (h->gene < 0) return;
	for (int k = 0; k < h->n_tied && k < VDJX_ANNOT_TIED; k++) fprintf(fp, "%s%s", k ? "," : "", g->names[h->tied[k]]);
}

static void put_cigar(FILE* fp, const vdjx_annot_hit* h, int m) {
	if (h->gene < 0 || h->score <= 0 || h->n_runs > VDJX_ANNOT_RUNS) return;
	if (h->seq_start > 1) fprintf(fp, "%dS", h->seq_start - 1);
	if (h->germ_start > 1) fprintf(fp, "%dN", h->germ_start - 1);
	for (int k = 0; k < h->n_runs; k++) fprintf(fp, "%u%c", h->runs[k] >> 4, "MID"[h->runs[k] & 15u]);
	if (h->seq_end < m) fprintf(fp, "%dS", m - h->seq_end);
}

static void put_hit(FILE* fp, const vdjx_annot_hit* h) {
	if (h->gene < 0) { fputs("\t\t\t\t\t\t", fp); return; }
	fprintf(fp, "\t%d", h->score);
	if (h->score <= 0) { fputs("\t\t\t\t\t", fp); return; }
	const int d = h->matches + h->mismatches + h->ins + h->del;
	fprintf(fp, "\t%.4f\t%d\t%d\t%d\t%d", (double) h->matches / d, h->seq_start, h->seq_end, h->germ_start, h->germ_end);
}

/* the junction: the text after the id's second '_', at its first occurrence in the contig -> its 0-based start (or -1); *jn, *jl: the text */
static long junction_at(const char* id, const char* s, int len, const char** jn_out, size_t* jl_out) {
	const char* u1 = strchr(id, '_');
	const char* jn = u1 ? strchr(u1 + 1, '_') : NULL;
	jn = jn && jn[1] ? jn + 1 : NULL;
	const size_t jl = jn ? strlen(jn) : 0;
	long p = -1;
	if (jn && jl <= (size_t) len)
		for (long q = 0; q + (long) jl <= len; q++)
			if (!memcmp(s + q, jn, jl)) { p = q; break; }
	*jn_out = jn;
	*jl_out = jl;
	return p;
}

/* the V / J hits of every contig (vdjx_annotate against the germlines of ig_vdj.fa / --vdjf), kept for the tables */
static int annot_run(hook_ud* u, const char* contigs, size_t n, int len) {
	u->germ = (germ_set*) calloc(1, sizeof(germ_set));
	if (germ_read(u->c->vdj_fasta, u->germ, u->c->airr ? "--airr: cannot read the germline FASTA" : u->c->clones ? "--clones: cannot read the germline FASTA" : u->c->lineages ? "--lineages: cannot read the germline FASTA" : u->c->mutations ? "--mutations: cannot read the germline FASTA" : u->c->selection ? "--selection: cannot read the germline FASTA" : "--targeting-model: cannot read the germline FASTA")) return -1;
	const germ_set* g = u->germ;
	for (size_t r = 0; r < g->n; r++) {
		if (g->cls[r] == 'V' || g->cls[r] == 'J') continue;
		if (g->cls[r] == 'D') u->a_skip_d++; else u->a_skip_other++;
	}
	u->hv = (vdjx_annot_hit*) calloc(n + 1, sizeof(vdjx_annot_hit));
	u->hj = (vdjx_annot_hit*) calloc(n + 1, sizeof(vdjx_annot_hit));
	const vdjx_annot_params ap = {2, 3, 5, 2, 40, 20};
	int rc = vdjx_germline_load(u->gx, g->seqs, g->off, g->cls, g->n);
	if (!rc && n) rc = vdjx_annotate(u->gx, contigs, n, len, &ap, u->hv, u->hj);
	if (rc) fprintf(stderr, "%s: %s\n", u->c->airr ? "--airr" : u->c->clones ? "--clones" : u->c->lineages ? "--lineages" : u->c->mutations ? "--mutations" : u->c->selection ? "--selection" : "--targeting-model", vdjx_last_error());
	return rc;
}

/* the window of --d-calls (include/vdjx.h, vdjx_dcall): the bases strictly between a V and a J hit -> its length (0: none), *start 0-based;
 * *over: more than VDJX_DCALL_WINDOW bases lie between the hits (no window) */
static int d_window(const vdjx_annot_hit* v, const vdjx_annot_hit* j, int32_t* start, int* over) {
	*start = 0;
	*over = 0;
	if (!(v->gene >= 0 && v->score > 0 && j->gene >= 0 && j->score > 0)) return 0;
	const int l = j->seq_start - 1 - v->seq_end;
	if (l <= 0) return 0;
	if (l > VDJX_DCALL_WINDOW) { *over = 1; return 0; }
	*start = v->seq_end;
	return l;
}

/* --d-calls: the D hits of every contig (vdjx_dcall: the window between its V and its J hit against the class-D records annot_run read) */
static int dcall_run(hook_ud* u, const char* contigs, size_t n, int len) {
	const germ_set* g = u->germ;
	germ_set* d = u->dset = (germ_set*) calloc(1, sizeof(germ_set));
	d->off = (uint64_t*) calloc(g->n + 1, sizeof(uint64_t));
	d->names = (char**) calloc(g->n + 1, sizeof(char*));
	d->seqs = (char*) malloc(g->bytes + 1);
	for (size_t r = 0; r < g->n; r++) {
		if (g->cls[r] != 'D') continue;
		const size_t l = (size_t) (g->off[r + 1] - g->off[r]);
		memcpy(d->seqs + d->bytes, g->seqs + g->off[r], l);
		d->bytes += l;
		d->names[d->n++] = g->names[r];
		d->off[d->n] = d->bytes;
	}
	u->hd = (vdjx_annot_hit*) calloc(n + 1, sizeof(vdjx_annot_hit));
	int32_t* ws = (int32_t*) calloc(n + 1, sizeof(int32_t));
	int32_t* wl = (int32_t*) calloc(n + 1, sizeof(int32_t));
	for (size_t i = 0; i < n; i++) {
		int over;
		wl[i] = d_window(u->hv + i, u->hj + i, ws + i, &over);
		u->d_windows += wl[i] > 0;
		u->d_over += (size_t) over;
	}
	const vdjx_dcall_params dp = {2, 3, 5, 2, 22};
	int rc = vdjx_dsegment_load(u->gx, d->seqs, d->off, d->n);
	if (!rc && n) rc = vdjx_dcall(u->gx, contigs, n, len, ws, wl, &dp, u->hd, NULL);
	if (rc) fprintf(stderr, "--d-calls: %s\n", vdjx_last_error());
	for (size_t i = 0; !rc && i < n; i++) { u->d_contigs++; u->d_called += u->hd[i].gene >= 0; }
	free(ws);
	free(wl);
	return rc;
}

/* --d-calls: the ten columns after j_germline_end: the D hit's six cells, then np1 (V's end to D's start), np2 (D's end to J's start) and
 * their lengths; without a D call np1 is the whole gap between the V and the J hit, without a V or a J hit the four cells are empty */
static void put_np(FILE* fp, const char* s, const vdjx_annot_hit* v, const vdjx_annot_hit* d, const vdjx_annot_hit* j) {
	put_hit(fp, d);
	if (!(v->gene >= 0 && v->score > 0 && j->gene >= 0 && j->score > 0)) { fputs("\t\t\t\t", fp); return; }
	const int hasd = d->gene >= 0 && d->score > 0;
	const int a0 = v->seq_end, a1 = hasd ? d->seq_start - 1 : j->seq_start - 1;       /* np1: 0-based [a0, a1) */
	const int b0 = hasd ? d->seq_end : 0, b1 = hasd ? j->seq_start - 1 : 0;            /* np2 */
	const int l1 = a1 > a0 ? a1 - a0 : 0, l2 = b1 > b0 ? b1 - b0 : 0;
	fprintf(fp, "\t%.*s\t%d\t%.*s\t%d", l1, s + a0, l1, l2, s + b0, l2);
}

static int airr_table(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) {
	const germ_set g = *u->germ;
	const vdjx_annot_hit *hv = u->hv, *hj = u->hj;
	int rc = 0;
	FILE* fp = fopen(u->c->airr, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->airr); rc = -1; }
	if (fp) {
		fputs("sequence_id\tsequence\trev_comp\tproductive\tv_call\td_call\tj_call\tsequence_alignment\tgermline_alignment\tjunction\tjunction_aa\t"
		      "cdr3\tcdr3_aa\tvj_in_frame\tstop_codon\tv_cigar\td_cigar\tj_cigar\tv_score\tv_identity\tv_sequence_start\tv_sequence_end\t"
		      "v_germline_start\tv_germline_end\tj_score\tj_identity\tj_sequence_start\tj_sequence_end\tj_germline_start\tj_germline_end", fp);
		if (u->c->d_calls)
			fputs("\td_score\td_identity\td_sequence_start\td_sequence_end\td_germline_start\td_germline_end\tnp1\tnp1_length\tnp2\tnp2_length", fp);
		if (u->c->lineages) fputs("\tclone_id", fp);
		fputs(u->c->quant ? "\texpected_count\n" : "\n", fp);
		for (size_t i = 0; i < n; i++) {
			const char* s = contigs + i * (size_t) len;
			const vdjx_annot_hit *v = hv + i, *j = hj + i;
			const char* jn;
			size_t jl;
			const long p = junction_at(ids[i], s, len, &jn, &jl);
			const size_t JL = p >= 0 ? jl : 0;
			const int hasv = v->gene >= 0 && v->score > 0, hasj = j->gene >= 0 && j->score > 0;
			const int inframe = p >= 0 && hasv && JL % 3 == 0 && (p - (v->seq_start - 1) + (v->germ_start - 1)) % 3 == 0;
			int stop = 0;
			if (p >= 0 && hasv && hasj)
				for (long q = p % 3; q + 2 <= j->seq_end - 1; q += 3)
					if (q >= v->seq_start - 1 && codon_aa(s + q) == '*') { stop = 1; break; }
			const int prod = hasv && hasj && inframe && !stop;
			u->a_contigs++;
			u->a_v += v->gene >= 0;
			u->a_j += j->gene >= 0;
			u->a_prod += prod;
			u->a_trunc += (v->gene >= 0 && v->n_runs > VDJX_ANNOT_RUNS) + (j->gene >= 0 && j->n_runs > VDJX_ANNOT_RUNS);
			fprintf(fp, "%s\t%.*s\tF\t%c\t", ids[i], len, s, prod ? 'T' : 'F');
			put_call(fp, v, &g);
			fputc('\t', fp);
			if (u->c->d_calls) put_call(fp, u->hd + i, u->dset);
			fputc('\t', fp);
			put_call(fp, j, &g);
			if (u->c->mutations) {               /* mut_run's rows: the contig and its germline, column by column */
				const int cols = (int) (u->mu_off[i + 1] - u->mu_off[i]);
				fprintf(fp, "\t%.*s\t%.*s\t", cols, cols ? u->mu_seq + u->mu_off[i] : "", cols, cols ? u->mu_germ + u->mu_off[i] : "");
			} else fputs("\t\t\t", fp);
			fprintf(fp, "%.*s\t", (int) JL, p >= 0 ? s + p : "");
			put_aa(fp, p >= 0 ? s + p : "", JL);
			const size_t cl = JL >= 6 ? JL - 6 : 0;
			fprintf(fp, "\t%.*s\t", (int) cl, cl ? s + p + 3 : "");
			put_aa(fp, cl ? s + p + 3 : "", cl);
			fprintf(fp, "\t%c\t%c\t", inframe ? 'T' : 'F', stop ? 'T' : 'F');
			put_cigar(fp, v, len);
			fputc('\t', fp);
			if (u->c->d_calls) put_cigar(fp, u->hd + i, len);
			fputc('\t', fp);
			put_cigar(fp, j, len);
			put_hit(fp, v);
			put_hit(fp, j);
			if (u->c->d_calls) put_np(fp, s, v, u->hd + i, j);
			if (u->c->lineages) { if (u->lin_clone[i] >= 0) fprintf(fp, "\tlin_%d", u->lin_clone[i] + 1); else fputc('\t', fp); }
			if (u->c->quant) fprintf(fp, "\t%.2f", u->qcnt ? u->qcnt[i] : 0.0);
			fputc('\n', fp);
		}
		if (fclose(fp)) { fprintf(stderr, "cannot write %s\n", u->c->airr); rc = -1; }
	}
	return rc;
}

/* ---- --isotypes / --clones (the model: include/vdjx.h, vdjx_isotype; the name rules: vdjer_amd/annot.py) ----------------------------- */
/* a comma-joined list of distinct items in order of first appearance */
typedef struct { char* s; size_t n, cap, cnt; } slist;

static void sl_add(slist* b, const char* item, size_t il) {
	size_t at = 0;
	for (size_t k = 0; k < b->cnt; k++) {
		size_t e = at;
		while (e < b->n && b->s[e] != ',') e++;
		if (e - at == il && !memcmp(b->s + at, item, il)) return;
		at = e + 1;
	}
	if (b->n + il + 2 > b->cap) { b->cap = 2 * (b->n + il + 2); b->s = (char*) realloc(b->s, b->cap); }
	if (b->cnt) b->s[b->n++] = ',';
	memcpy(b->s + b->n, item, il);
	b->n += il;
	b->s[b->n] = 0;
	b->cnt++;
}

static const char* sl_str(const slist* b) { return b->s ? b->s : ""; }

/* subtypes: per called name the first four characters of the text before its first '*' (IGHG1*01 -> IGHG) */
static void subtypes_of(const vdjx_annot_hit* h, const germ_set* g, slist* out) {
	out->n = out->cnt = 0;
	if (out->s) out->s[0] = 0;
	if (h->gene < 0) return;
	for (int k = 0; k < h->n_tied && k < VDJX_ANNOT_TIED; k++) {
		const char* nm = g->names[h->tied[k]];
		size_t l = strcspn(nm, "*");
		sl_add(out, nm, l < 4 ? l : 4);
	}
}

/* get_vq_gene (collect_vdjer_stats.py): per called name the text before '*', every 'D' deleted, then what lies before a second '-' */
static void vq_gene_of(const vdjx_annot_hit* h, const germ_set* g, slist* out) {
	out->n = out->cnt = 0;
	if (out->s) out->s[0] = 0;
	if (h->gene < 0) return;
	for (int k = 0; k < h->n_tied && k < VDJX_ANNOT_TIED; k++) {
		const char* nm = g->names[h->tied[k]];
		const size_t l = strcspn(nm, "*");
		char* t = (char*) malloc(l + 1);
		size_t tl = 0;
		int dashes = 0;
		for (size_t q = 0; q < l; q++) {
			if (nm[q] == 'D') continue;
			if (nm[q] == '-' && ++dashes == 2) break;
			t[tl++] = nm[q];
		}
		sl_add(out, t, tl);
		free(t);
	}
}

/* the isotype hits of every contig (vdjx_isotype against the records of --cfa), kept for the tables */
static int iso_run(hook_ud* u, const char* contigs, size_t n, int len) {
	u->cst = (germ_set*) calloc(1, sizeof(germ_set));
	if (germ_read(u->c->cfa, u->cst, "--cfa: cannot read the constant-region FASTA")) return -1;
	u->hc = (vdjx_annot_hit*) calloc(n + 1, sizeof(vdjx_annot_hit));
	const vdjx_isotype_params ip = {2, 3, 5, 2, 48, 48};
	int rc = vdjx_constant_load(u->gx, u->cst->seqs, u->cst->off, u->cst->n);
	if (!rc && n) rc = vdjx_isotype(u->gx, contigs, n, len, &ip, u->hc, NULL);
	if (rc) fprintf(stderr, "%s: %s\n", u->c->isotypes ? "--isotypes" : "--clones", vdjx_last_error());
	for (size_t i = 0; !rc && i < n; i++) { u->i_contigs++; u->i_called += u->hc[i].gene >= 0; }
	return rc;
}

static int isotypes_table(hook_ud* u, const char* const* ids, size_t n, int len) {
	FILE* fp = fopen(u->c->isotypes, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->isotypes); return -1; }
	fputs("sequence_id\tisotype\tc_call\tc_score\tc_identity\tc_sequence_start\tc_sequence_end\tc_germline_start\tc_germline_end\tc_cigar\n", fp);
	slist sub;
	memset(&sub, 0, sizeof sub);
	for (size_t i = 0; i < n; i++) {
		const vdjx_annot_hit* h = u->hc + i;
		subtypes_of(h, u->cst, &sub);
		fprintf(fp, "%s\t%s\t", ids[i], sl_str(&sub));
		put_call(fp, h, u->cst);
		put_hit(fp, h);
		fputc('\t', fp);
		put_cigar(fp, h, len);
		fputc('\n', fp);
	}
	free(sub.s);
	if (fclose(fp)) { fprintf(stderr, "cannot write %s\n", u->c->isotypes); return -1; }
	return 0;
}

/* --clones: the table collect_vdjer_stats.py | cluster_results.py make of RSEM's, V-QUEST's and the isotype step's outputs, for this
 * sample: a row per contig whose printed expected_count is >= 1, that has a V call and whose junction is found in it with a non-empty
 * translation; a cluster id per distinct (isotype, aa cdr3, vgene, jgene) in order of first appearance */
static int clones_table(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) {
	FILE* fp = fopen(u->c->clones, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->clones); return -1; }
	fputs("sample\tsequence\tcdr3\texpected_counts\tseq_id\tisotype\tvregion_identity\taa_cdr3\tvgene\tjgene\ttotal_count\tcluster\n", fp);
	slist sub, vg, jg;
	memset(&sub, 0, sizeof sub); memset(&vg, 0, sizeof vg); memset(&jg, 0, sizeof jg);
	char** keys = NULL;
	size_t nkeys = 0, kcap = 0;
	for (size_t i = 0; i < n; i++) {
		const char* s = contigs + i * (size_t) len;
		const vdjx_annot_hit *v = u->hv + i, *j = u->hj + i;
		char cnt[64];
		snprintf(cnt, sizeof cnt, "%.2f", u->qcnt ? u->qcnt[i] : 0.0);
		const char* jn;
		size_t jl;
		const long p = junction_at(ids[i], s, len, &jn, &jl);
		if (!(atof(cnt) >= 1.0) || v->gene < 0 || p < 0 || jl < 3) continue;
		const int d = v->matches + v->mismatches + v->ins + v->del;
		char* aa = (char*) malloc(jl / 3 + 1);
		size_t al = 0;
		for (size_t q = 0; q + 3 <= jl; q += 3) aa[al++] = codon_aa(s + p + q);
		aa[al] = 0;
		const int called = u->hc && u->hc[i].gene >= 0;
		if (called) subtypes_of(u->hc + i, u->cst, &sub);
		const char* iso = called ? sl_str(&sub) : "N/A";
		vq_gene_of(v, u->germ, &vg);
		vq_gene_of(j, u->germ, &jg);
		const char* jgene = j->gene >= 0 ? sl_str(&jg) : "N/A";
		const size_t kl = strlen(iso) + al + strlen(sl_str(&vg)) + strlen(jgene) + 4;
		char* key = (char*) malloc(kl);
		snprintf(key, kl, "%s\t%s\t%s\t%s", iso, aa, sl_str(&vg), jgene);
		size_t k = 0;
		while (k < nkeys && strcmp(keys[k], key)) k++;
		if (k == nkeys) {
			if (nkeys + 1 > kcap) { kcap = kcap ? 2 * kcap : 64; keys = (char**) realloc(keys, kcap * sizeof(char*)); }
			keys[nkeys++] = key;
		} else free(key);
		fprintf(fp, "%s\t%.*s\t%s\t%s\t%s\t%s\t", u->c->sample, len, s, jn, cnt, ids[i], iso);
		if (d > 0) fprintf(fp, "%.2f", 100.0 * ((double) v->matches / d)); else fputs("N/A", fp);
		fprintf(fp, "\t%s\t%s\t%s\t%s\tcls_%zu\n", aa, sl_str(&vg), jgene, u->c->total_count ? u->c->total_count : "N/A", k + 1);
		free(aa);
		u->c_rows++;
	}
	u->c_clusters = nkeys;
	for (size_t k = 0; k < nkeys; k++) free(keys[k]);
	free(keys); free(sub.s); free(vg.s); free(jg.s);
	if (fclose(fp)) { fprintf(stderr, "cannot write %s\n", u->c->clones); return -1; }
	return 0;
}

/* --lineages: the contigs grouped into clonal lineages (the model: include/vdjx.h, vdjx_lineage; the inputs: lineage_inputs of
 * vdjer_amd/annot.py).  A contig is eligible when it has a V and a J call and its junction is found in it with 3 .. 255 bases; its group is
 * the index, by first appearance, of its (vgene, jgene) pair as --clones prints them.  A row per contig: clone_id lin_<k>, vgene, jgene,
 * junction_length, dist_nearest (the smallest non-zero distance inside the bucket over the length), clone_size and, when the quant step ran,
 * clone_expected_count: the sum of the members' expected_count as printed (two decimals each), so that the tables add up */
/* one pair pass at u->lin_num / u->c->lin_den, under --lineage-link's linkage */
static int lineage_pass(hook_ud* u, const char* cat, const uint64_t* off, const uint32_t* grp, size_t n, int32_t* near) {
	const vdjx_lineage_params lp = {u->lin_num, u->c->lin_den};
	const vdjx_lineage_model_params lmp = {u->lin_num, u->c->lin_den, u->c->lin_sym};
	const vdjx_lineage_link_params lkp = {u->lin_num, u->c->lin_den, u->c->lin_sym, u->c->lin_linkage};
	const int rc = u->c->lin_linkage ? vdjx_lineage_link(u->gx, cat, off, grp, n, &lkp, u->c->lin_table, u->lin_clone, near, &u->li, &u->lki)
	             : u->c->lin_table   ? vdjx_lineage_model(u->gx, cat, off, grp, n, &lmp, u->c->lin_table, u->lin_clone, near, &u->li)
	                              : vdjx_lineage(u->gx, cat, off, grp, n, &lp, u->lin_clone, near, &u->li);
	if (rc) fprintf(stderr, "--lineages: %s\n", vdjx_last_error());
	return rc;
}

static int lineage_run(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) {
	FILE* fp = fopen(u->c->lineages, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->lineages); return -1; }
	FILE* tfp = u->c->lin_threshold ? fopen(u->c->lin_threshold, "w") : NULL;
	if (u->c->lin_threshold && !tfp) { fprintf(stderr, "cannot write %s\n", u->c->lin_threshold); fclose(fp); return -1; }
	const int counted = u->c->quant || u->c->clones;
	const uint32_t B = counted && u->qboot ? u->c->qb_b : 0;      /* --quant-boot: clone_count_sd */
	char* cat = (char*) malloc(n * (size_t) VDJX_LINEAGE_MAXLEN + 1);
	uint64_t* off = (uint64_t*) calloc(n + 1, sizeof(uint64_t));
	uint32_t* grp = (uint32_t*) calloc(n + 1, sizeof(uint32_t));
	int32_t* near = (int32_t*) calloc(n + 1, sizeof(int32_t));
	char** vgs = (char**) calloc(n + 1, sizeof(char*));
	char** jgs = (char**) calloc(n + 1, sizeof(char*));
	u->lin_clone = (int32_t*) calloc(n + 1, sizeof(int32_t));
	slist vg, jg;
	memset(&vg, 0, sizeof vg); memset(&jg, 0, sizeof jg);
	char** keys = NULL;
	size_t nkeys = 0, kcap = 0, tot = 0;
	for (size_t i = 0; i < n; i++) {
		const vdjx_annot_hit *v = u->hv + i, *j = u->hj + i;
		vq_gene_of(v, u->germ, &vg);
		vq_gene_of(j, u->germ, &jg);
		vgs[i] = strdup(sl_str(&vg));
		jgs[i] = strdup(sl_str(&jg));
		const char* jn;
		size_t jl;
		const long p = junction_at(ids[i], contigs + i * (size_t) len, len, &jn, &jl);
		grp[i] = VDJX_LINEAGE_NONE;
		if (v->gene >= 0 && j->gene >= 0 && p >= 0 && jl >= 3 && jl <= VDJX_LINEAGE_MAXLEN) {
			const size_t kl = strlen(vgs[i]) + strlen(jgs[i]) + 2;
			char* key = (char*) malloc(kl);
			snprintf(key, kl, "%s\t%s", vgs[i], jgs[i]);
			size_t k = 0;
			while (k < nkeys && strcmp(keys[k], key)) k++;
			if (k == nkeys) {
				if (nkeys + 1 > kcap) { kcap = kcap ? 2 * kcap : 64; keys = (char**) realloc(keys, kcap * sizeof(char*)); }
				keys[nkeys++] = key;
			} else free(key);
			grp[i] = (uint32_t) k;
			memcpy(cat + tot, jn, jl);
			tot += jl;
			u->l_eligible++;
		}
		off[i + 1] = tot;
		u->l_contigs++;
	}
	int rc = lineage_pass(u, cat, off, grp, n, near);
	/* --lineage-threshold: the valley of the nearest distances of that pass (the model: include/vdjx.h, vdjx_lineage_threshold); where one is
	 * found and it is not the threshold the pass ran with, the pass runs once more with it.  Otherwise --lineage-dist stands */
	u->thr_fallback = u->lin_num;
	u->thr_passes = 1;
	if (!rc && tfp) {
		const vdjx_threshold_params tp = {200, 5, 1, 2, 10};
		uint32_t* lens = (uint32_t*) calloc(n + 1, sizeof(uint32_t));
		uint32_t* hist = (uint32_t*) calloc(VDJX_THRESHOLD_GRID + 1, sizeof(uint32_t));
		uint64_t* dens = (uint64_t*) calloc(VDJX_THRESHOLD_GRID + 1, sizeof(uint64_t));
		for (size_t i = 0; i < n; i++) lens[i] = (uint32_t) (off[i + 1] - off[i]);
		rc = vdjx_lineage_threshold(u->gx, near, lens, n, u->c->lin_table ? 2000u : 1u, &tp, hist, dens, NULL, &u->thi);
		if (rc) fprintf(stderr, "--lineage-threshold: %s\n", vdjx_last_error());
		if (!rc && u->thi.status == VDJX_THRESHOLD_FOUND && (int) u->thi.threshold != u->lin_num) {
			u->lin_num = (int) u->thi.threshold;           /* (lin_den is 10000, the grid's unit) */
			rc = lineage_pass(u, cat, off, grp, n, near);
			u->thr_passes = 2;
		}
		if (!rc) {
			static const char* const names[5] = {"found", "too few values", "no scale", "one mode", "shallow valley"};
			const vdjx_threshold_info* t = &u->thi;
			fprintf(tfp, "# status\t%s\n# values\t%u\n# distinct\t%u\n# bandwidth\t%.3f\n", names[t->status <= 4 ? t->status : 0], t->values, t->distinct, t->k / 1000.0);
			fprintf(tfp, "# peak1\t%.4f\t%.4f\t%llu\n# peak2\t%.4f\t%.4f\t%llu\n", t->p1_first / 10000.0, t->p1_last / 10000.0, (unsigned long long) t->y1,
			        t->p2_first / 10000.0, t->p2_last / 10000.0, (unsigned long long) t->y2);
			fprintf(tfp, "# valley\t%.4f\t%.4f\t%llu\n# threshold\t%.4f\n# scale\t%u\n", t->t_first / 10000.0, t->t_last / 10000.0, (unsigned long long) t->m,
			        u->lin_num / 10000.0, 1u << 30);
			fputs("dist\tcount\tdensity\n", tfp);
			for (uint32_t g = 0; g <= VDJX_THRESHOLD_GRID; g++) fprintf(tfp, "%.4f\t%u\t%llu\n", g / 10000.0, hist[g], (unsigned long long) dens[g]);
		}
		free(lens); free(hist); free(dens);
	}
	if (tfp && fclose(tfp)) { fprintf(stderr, "cannot write %s\n", u->c->lin_threshold); rc = -1; }
	if (!rc && u->c->lin_table) u->lin_walked = vdjx_stat(u->gx, "lineage_model_walked");
	const double unit = u->c->lin_table ? 2000.0 : 1.0;      /* dist_nearest: in mean mismatches per base under a model */
	if (!rc) {
		size_t* size = (size_t*) calloc((size_t) u->li.clones + 1, sizeof(size_t));
		double* sum = (double*) calloc((size_t) u->li.clones + 1, sizeof(double));
		for (size_t i = 0; i < n; i++) {
			if (u->lin_clone[i] < 0) continue;
			char cnt[64];
			snprintf(cnt, sizeof cnt, "%.2f", u->qcnt ? u->qcnt[i] : 0.0);
			size[u->lin_clone[i]]++;
			sum[u->lin_clone[i]] += atof(cnt);
		}
		/* clone_count_sd: per lineage and replicate the members' unrounded replicate counts added in contig order, then the sd of
		 * vdjx_quant_boot_summary over the replicates */
		const size_t nk = (size_t) u->li.clones;
		double* csd = (double*) calloc(nk + 1, sizeof(double));
		if (B) {
			double* cb = (double*) calloc((size_t) B * nk + 1, sizeof(double));
			for (uint32_t r = 0; r < B; r++)
				for (size_t i = 0; i < n; i++)
					if (u->lin_clone[i] >= 0) cb[(size_t) r * nk + (size_t) u->lin_clone[i]] += u->qboot[(size_t) r * n + i];
			vdjx_quant_boot_summary(cb, B, nk, NULL, csd, NULL, NULL);
			free(cb);
		}
		fprintf(fp, "sequence_id\tclone_id\tvgene\tjgene\tjunction_length\tdist_nearest\tclone_size%s%s\n", counted ? "\tclone_expected_count" : "",
		        B ? "\tclone_count_sd" : "");
		for (size_t i = 0; i < n; i++) {
			const int32_t k = u->lin_clone[i];
			const uint64_t L = off[i + 1] - off[i];
			if (k < 0) { fprintf(fp, "%s\t\t%s\t%s\t\t\t%s%s\n", ids[i], vgs[i], jgs[i], counted ? "\t" : "", B ? "\t" : ""); continue; }
			fprintf(fp, "%s\tlin_%d\t%s\t%s\t%llu\t", ids[i], k + 1, vgs[i], jgs[i], (unsigned long long) L);
			if (near[i] >= 0) fprintf(fp, "%.4f", (double) near[i] / (unit * (double) L));
			fprintf(fp, "\t%zu", size[k]);
			if (counted) fprintf(fp, "\t%.2f", sum[k]);
			if (B) fprintf(fp, "\t%.2f", csd[k]);
			fputc('\n', fp);
		}
		free(size); free(sum); free(csd);
	}
	for (size_t i = 0; i < n; i++) { free(vgs[i]); free(jgs[i]); }
	for (size_t k = 0; k < nkeys; k++) free(keys[k]);
	free(keys); free(vgs); free(jgs); free(vg.s); free(jg.s); free(cat); free(off); free(grp); free(near);
	if (fclose(fp)) { fprintf(stderr, "cannot write %s\n", u->c->lineages); return -1; }
	return rc;
}

/* --trees: the tree inside every lineage (the model: include/vdjx.h, vdjx_tree; the inputs: tree_inputs of vdjer_amd/annot.py).  The clones
 * are lineage_run's; a member's anchor is where its junction starts and its priority its V hit's mismatches + ins + del, so the member closest
 * to its germline V is the root.  A row per contig: clone_id lin_<k>, parent_id, dist_parent (both empty for a root), depth, children,
 * v_mutations, window_start (0-based, in this contig) and window_length of the lineage's common window; only sequence_id for a contig
 * that is in no lineage.  --tree-support B: one more column, support, the share of B jackknife replicates whose tree has the edge to
 * parent_id (vdjx_tree_support on vdjx_tree's parents), empty for a root */
static int tree_run(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) {
	FILE* fp = fopen(u->c->trees, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->trees); return -1; }
	fprintf(fp, "sequence_id\tclone_id\tparent_id\tdist_parent\tdepth\tchildren\tv_mutations\twindow_start\twindow_length%s\n", u->c->ts_b ? "\tsupport" : "");
	int32_t* anchor = (int32_t*) calloc(n + 1, sizeof(int32_t));
	uint32_t* prio = (uint32_t*) calloc(n + 1, sizeof(uint32_t));
	int32_t* out = (int32_t*) calloc(4 * n + 1, sizeof(int32_t));
	int32_t *parent = out, *dist = out + n, *depth = out + 2 * n, *support = out + 3 * n;
	const size_t nk = (size_t) u->li.clones + 1;
	int32_t* before = (int32_t*) malloc(nk * sizeof(int32_t));       /* per lineage: the window's bases before the anchor, and from it on */
	int32_t* after = (int32_t*) malloc(nk * sizeof(int32_t));
	size_t* kids = (size_t*) calloc(n + 1, sizeof(size_t));
	for (size_t k = 0; k < nk; k++) before[k] = after[k] = len;
	for (size_t i = 0; i < n; i++) {
		const int32_t k = u->lin_clone[i];
		if (k < 0) continue;
		const vdjx_annot_hit* v = u->hv + i;
		const char* jn;
		size_t jl;
		anchor[i] = (int32_t) junction_at(ids[i], contigs + i * (size_t) len, len, &jn, &jl);
		prio[i] = (uint32_t) (v->mismatches + v->ins + v->del);
		if (anchor[i] < before[k]) before[k] = anchor[i];
		if (len - anchor[i] < after[k]) after[k] = len - anchor[i];
	}
	int rc = vdjx_tree(u->gx, contigs, n, len, u->lin_clone, anchor, prio, parent, dist, depth, &u->ti);
	if (rc) fprintf(stderr, "--trees: %s\n", vdjx_last_error());
	if (!rc && u->c->ts_b) {
		const vdjx_tree_support_params tp = {u->c->ts_b, u->c->ts_seed};
		rc = vdjx_tree_support(u->gx, contigs, n, len, u->lin_clone, anchor, parent, &tp, support, &u->tsi);
		if (rc) fprintf(stderr, "--tree-support: %s\n", vdjx_last_error());
	}
	if (!rc) {
		for (size_t i = 0; i < n; i++)
			if (parent[i] >= 0) kids[parent[i]]++;
		for (size_t i = 0; i < n; i++) {
			const int32_t k = u->lin_clone[i];
			if (k < 0) { fprintf(fp, "%s\t\t\t\t\t\t\t\t%s\n", ids[i], u->c->ts_b ? "\t" : ""); continue; }
			fprintf(fp, "%s\tlin_%d\t", ids[i], k + 1);
			if (parent[i] >= 0) fprintf(fp, "%s\t%d", ids[parent[i]], dist[i]); else fputc('\t', fp);
			fprintf(fp, "\t%d\t%zu\t%u\t%d\t%d", depth[i], kids[i], prio[i], anchor[i] - before[k], before[k] + after[k]);
			if (u->c->ts_b && parent[i] >= 0) fprintf(fp, "\t%.4f", (double) support[i] / (double) u->c->ts_b);
			else if (u->c->ts_b) fputc('\t', fp);
			fputc('\n', fp);
		}
	}
	free(anchor); free(prio); free(out); free(before); free(after); free(kids);
	if (fclose(fp)) { fprintf(stderr, "cannot write %s\n", u->c->trees); return -1; }
	return rc;
}

/* --trees-nj: the neighbour-joining tree inside every lineage, with its inferred ancestors (the model: include/vdjx.h, vdjx_tree_nj; in
 * Python: tests/tree_nj_model.py).  The clones, anchors and priorities are tree_run's.  A row per node: lineages in number order; inside one
 * the members in contig order, then the inferred nodes lin_<k>_a<j> (j from 1) in creation order; parent_id and mutations empty for a root;
 * branch_length = length / 65536; sequence: the node's window -- the observed characters of a member, Fitch's states of an inferred node.  A
 * contig in no lineage has no row.  --trees-newick: a line per lineage of two and more members, lin_<k>, a tab, the tree (vdjx_newick.h) */
typedef struct { const char* const* ids; const int32_t* clone; const uint32_t* number; size_t n; } nj_names;
static void nj_label(FILE* fp, size_t s, void* ud) {
	const nj_names* q = (const nj_names*) ud;
	if (s < q->n) fputs(q->ids[s], fp);
	else fprintf(fp, "lin_%d_a%u", q->clone[s] + 1, q->number[s - q->n] + 1);
}

/* mp: --trees-mp, --trees-mp-newick instead -- vdjx_tree_mp from vdjx_tree_nj's tree (the model: tests/tree_mp_model.py); the same rows,
 * branch_length the node's mutations */
static int tree_nodes_run(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len, int mp) {
	const char *table = mp ? u->c->trees_mp : u->c->trees_nj, *lines = mp ? u->c->trees_mp_newick : u->c->trees_newick;
	const char *flag = mp ? "--trees-mp" : "--trees-nj", *flag_lines = mp ? "--trees-mp-newick" : "--trees-newick";
	FILE* fp = fopen(table, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", table); return -1; }
	FILE* np = lines ? fopen(lines, "w") : NULL;
	if (lines && !np) { fprintf(stderr, "cannot write %s\n", lines); fclose(fp); return -1; }
	fputs("clone_id\tnode_id\tparent_id\tbranch_length\tmutations\tdepth\tchildren\tobserved\tsequence\n", fp);
	int32_t* anchor = (int32_t*) calloc(n + 1, sizeof(int32_t));
	uint32_t* prio = (uint32_t*) calloc(n + 1, sizeof(uint32_t));
	const size_t nk = (size_t) u->li.clones + 1;
	int32_t* before = (int32_t*) malloc(nk * sizeof(int32_t));       /* per lineage: the window's bases before the anchor, and from it on */
	int32_t* after = (int32_t*) malloc(nk * sizeof(int32_t));
	size_t* first = (size_t*) calloc(nk + 1, sizeof(size_t));       /* per lineage: where its members start in member[] */
	size_t* member = (size_t*) calloc(n + 1, sizeof(size_t));
	for (size_t k = 0; k < nk; k++) before[k] = after[k] = len;
	for (size_t i = 0; i < n; i++) {
		const int32_t k = u->lin_clone[i];
		if (k < 0) continue;
		const vdjx_annot_hit* v = u->hv + i;
		const char* jn;
		size_t jl;
		anchor[i] = (int32_t) junction_at(ids[i], contigs + i * (size_t) len, len, &jn, &jl);
		prio[i] = (uint32_t) (v->mismatches + v->ins + v->del);
		if (anchor[i] < before[k]) before[k] = anchor[i];
		if (len - anchor[i] < after[k]) after[k] = len - anchor[i];
		first[k + 1]++;
	}
	for (size_t k = 0; k < nk; k++) first[k + 1] += first[k];
	{
		size_t* fill = (size_t*) malloc((nk + 1) * sizeof(size_t));
		for (size_t k = 0; k < nk; k++) fill[k] = first[k];
		for (size_t i = 0; i < n; i++)
			if (u->lin_clone[i] >= 0) member[fill[u->lin_clone[i]]++] = i;
		free(fill);
	}
	uint64_t nodes = n;
	int rc = n ? vdjx_tree_nj_nodes(u->lin_clone, n, &nodes) : 0;
	const size_t inner = (size_t) (nodes - n);
	int32_t* out = (int32_t*) calloc(4 * (size_t) nodes + 1, sizeof(int32_t));
	int32_t *parent = out, *mut = out + nodes, *depth = out + 2 * nodes, *cl = out + 3 * nodes;
	int64_t* length = (int64_t*) calloc((size_t) nodes + 1, sizeof(int64_t));
	char* anc = (char*) calloc(inner * (size_t) len + 1, 1);
	uint32_t* number = (uint32_t*) calloc(inner + 1, sizeof(uint32_t));
	size_t* kid_off = (size_t*) calloc((size_t) nodes + 2, sizeof(size_t));
	uint32_t* kid = (uint32_t*) calloc((size_t) nodes + 1, sizeof(uint32_t));
	if (!rc && !mp) rc = vdjx_tree_nj(u->gx, contigs, n, len, u->lin_clone, anchor, prio, parent, length, mut, depth, cl, anc, &u->tni);
	if (!rc && mp) {
		rc = vdjx_tree_mp(u->gx, contigs, n, len, u->lin_clone, anchor, prio, NULL, NULL, parent, mut, depth, cl, anc, &u->tmi);
		for (size_t s = 0; !rc && s < (size_t) nodes; s++) length[s] = cl[s] < 0 ? -1 : (parent[s] < 0 ? 0 : (int64_t) mut[s] * 65536);      /* an edge's length is its mutations */
	}
	if (rc) fprintf(stderr, "%s: %s\n", flag, vdjx_last_error());
	if (!rc && newick_children(parent, (size_t) nodes, kid_off, kid)) { fprintf(stderr, "%s: the parents are no forest\n", flag); rc = -1; }
	if (!rc) {
		for (size_t a = 1; a < inner; a++) number[a] = cl[n + a] == cl[n + a - 1] ? number[a - 1] + 1 : 0;
		const nj_names names = {ids, cl, number, n};
		size_t slot = n;                                             /* the lineage's first inferred node */
		for (size_t k = 0; k + 1 < nk; k++) {
			const size_t m = first[k + 1] - first[k], extra = m > 2 ? m - 2 : 0;
			const int w = before[k] + after[k];
			size_t root = 0;
			for (size_t q = 0; q < m + extra; q++) {
				const size_t s = q < m ? member[first[k] + q] : slot + (q - m);
				fprintf(fp, "lin_%zu\t", k + 1);
				nj_label(fp, s, (void*) &names);
				fputc('\t', fp);
				if (parent[s] >= 0) nj_label(fp, (size_t) parent[s], (void*) &names); else root = s;
				fprintf(fp, "\t%.4f\t", (double) length[s] / 65536.0);
				if (parent[s] >= 0) fprintf(fp, "%d", mut[s]);
				fprintf(fp, "\t%d\t%zu\t%c\t%.*s\n", depth[s], kid_off[s + 1] - kid_off[s], q < m ? 'T' : 'F', w,
				        q < m ? contigs + s * (size_t) len + (anchor[s] - before[k]) : anc + (s - n) * (size_t) len);
			}
			if (np && m >= 2) {
				fprintf(np, "lin_%zu\t", k + 1);
				if (newick_write(np, root, length, (size_t) nodes, kid_off, kid, nj_label, (void*) &names)) { fprintf(stderr, "%s: lineage %zu is no tree\n", flag_lines, k + 1); rc = -1; break; }
				fputc('\n', np);
			}
			slot += extra;
		}
	}
	free(anchor); free(prio); free(before); free(after); free(first); free(member); free(out); free(length); free(anc); free(number); free(kid_off); free(kid);
	if (np && fclose(np)) { fprintf(stderr, "cannot write %s\n", lines); fclose(fp); return -1; }
	if (fclose(fp)) { fprintf(stderr, "cannot write %s\n", table); return -1; }
	return rc;
}
static int tree_nj_run(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) { return tree_nodes_run(u, ids, contigs, n, len, 0); }
static int tree_mp_run(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) { return tree_nodes_run(u, ids, contigs, n, len, 1); }

/* --mutations: the germline rows and the V mutation counts of every contig (the model: include/vdjx.h, vdjx_mutations; the limit:
 * mutation_limit of vdjer_amd/annot.py).  V mutations are counted below the junction's start + 3, through the conserved Cys codon: what
 * follows is the CDR3.  The D hits of --d-calls are laid into the gap; the rows are kept for the --airr table. */
static int32_t* mutation_limits(const char* const* ids, const char* contigs, size_t n, int len) {
	int32_t* lim = (int32_t*) calloc(n + 1, sizeof(int32_t));
	for (size_t i = 0; i < n; i++) {
		const char* jn;
		size_t jl;
		const long p = junction_at(ids[i], contigs + i * (size_t) len, len, &jn, &jl);
		lim[i] = p >= 0 && p + 3 < len ? (int32_t) p + 3 : len;
	}
	return lim;
}

static int mut_run(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) {
	FILE* fp = fopen(u->c->mutations, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->mutations); return -1; }
	const germ_set g = *u->germ;
	const vdjx_annot_hit* hd = u->c->d_calls ? u->hd : NULL;
	u->mu_off = (uint64_t*) calloc(n + 1, sizeof(uint64_t));
	int32_t* lim = mutation_limits(ids, contigs, n, len);
	vdjx_mut_row* rows = (vdjx_mut_row*) calloc(n + 1, sizeof(vdjx_mut_row));
	char* mask = NULL;
	int rc = n ? vdjx_mutations_layout(u->hv, hd, u->hj, n, u->mu_off) : 0;
	if (!rc) {
		const size_t total = (size_t) u->mu_off[n];
		u->mu_seq = (char*) malloc(total + 1);
		u->mu_germ = (char*) malloc(total + 1);
		mask = (char*) malloc(total + 1);
		rc = vdjx_mutations(u->gx, contigs, n, len, u->hv, hd, u->hj, lim, u->mu_seq, u->mu_germ, mask, rows, &u->mi);
	}
	if (rc) fprintf(stderr, "--mutations: %s\n", vdjx_last_error());
	if (!rc) {
		fputs("sequence_id\tv_call\tj_call\tsequence_alignment\tgermline_alignment\tgermline_alignment_d_mask\tv_germline_codons\tmu_count_v_r\t"
		      "mu_count_v_s\tmu_count_v_stop\tmu_count_v_na\tmu_freq_v\tmu_count_j", fp);
		fputs(u->c->lineages ? "\tclone_id\n" : "\n", fp);
		for (size_t i = 0; i < n; i++) {
			const vdjx_mut_row* r = rows + i;
			fprintf(fp, "%s\t", ids[i]);
			put_call(fp, u->hv + i, &g);
			fputc('\t', fp);
			put_call(fp, u->hj + i, &g);
			if (r->flags & 1) {
				const int cols = r->cols;
				const uint64_t at = u->mu_off[i];
				fprintf(fp, "\t%.*s\t%.*s\t%.*s\t%d\t%d\t%d\t%d\t%d\t", cols, u->mu_seq + at, cols, u->mu_germ + at, cols, mask + at, r->v_codons, r->v_r,
				        r->v_s, r->v_stop, r->v_na);
				if (r->v_codons) fprintf(fp, "%.4f", (double) (r->v_r + r->v_s) / (double) (3 * r->v_codons));
				fprintf(fp, "\t%d", r->j_mis);
			} else fputs("\t\t\t\t\t\t\t\t\t\t", fp);
			if (u->c->lineages) { if (u->lin_clone[i] >= 0) fprintf(fp, "\tlin_%d", u->lin_clone[i] + 1); else fputc('\t', fp); }
			fputc('\n', fp);
		}
	}
	free(lim);
	free(rows);
	free(mask);
	if (fclose(fp) && !rc) { fprintf(stderr, "cannot write %s\n", u->c->mutations); return -1; }
	return rc;
}

/* --selection: the selection strength of the V segment's mutations (the model: include/vdjx.h, vdjx_selection), in the long format of
 * shazam's summarizeBaseline: a row per contig, per lineage of --lineages and for the sample, times the regions (v; fwr and cdr with
 * --v-regions).  The limit is --mutations'.  A V record without a --v-regions line has no regions: its contigs take no part. */
static void sel_rows(FILE* fp, const char* level, const char* id, const vdjx_sel_stat* st, uint32_t K) {
	for (uint32_t k = 0; k < K; k++) {
		const vdjx_sel_stat* s = st + k;
		const double sg = s->sigma > -0.00005 && s->sigma < 0.0 ? 0.0 : s->sigma;      /* (no "-0.0000") */
		fprintf(fp, "%s\t%s\t%s\t%u\t%llu\t%llu\t%llu\t%llu\t%.4f\t%.2f\t%.2f\t%.4f\n", level, id, K == 1 ? "v" : k ? "cdr" : "fwr", s->sequences,
		        (unsigned long long) s->x, (unsigned long long) (s->n - s->x), (unsigned long long) s->exp_r, (unsigned long long) s->exp_s, sg, s->lower, s->upper,
		        s->p_positive);
	}
}

/* --selection-combine mean: the posterior cells of the rows st[rows * K] from the members' densities (vdjx_selection_convolve over the
 * counts a vdjx_selection call returned); the counts of a row are the same in both, so the whole stat is taken.  The infos add up. */
static int sel_mean_rows(hook_ud* u, const vdjx_sel_counts* cnt, size_t n, uint32_t K, const int32_t* group, uint32_t G, vdjx_sel_stat* st, double* pdf) {
	vdjx_selconv_info ci;
	const int rc = vdjx_selection_convolve(u->gx, cnt, n, K, group, G, st, pdf, &ci);
	if (rc) { fprintf(stderr, "--selection-combine: %s\n", vdjx_last_error()); return rc; }
	u->sci.members += ci.members; u->sci.leaves += ci.leaves; u->sci.combines += ci.combines;
	u->sci.rows += ci.rows; u->sci.batches += ci.batches;
	if (ci.levels > u->sci.levels) u->sci.levels = ci.levels;
	return 0;
}

static double sel_no_minus_zero(double sg) { return sg > -0.00005 && sg < 0.0 ? 0.0 : sg; }

/* --selection-test: cdr against fwr for every lineage, the sample and the consensus sample (vdjx_selection_compare; the densities are the
 * chosen combine mode's).  st / pdf: the T rows of 2 regions in table order; a side without a contributing sequence leaves the cells empty. */
static int sel_test_write(const char* path, const char* const* level, char* const* id, size_t T, const vdjx_sel_stat* st, const double* pdf) {
	FILE* fp = fopen(path, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", path); return -1; }
	fputs("level\tid\tregion_a\tregion_b\tsigma_a\tsigma_b\tp_greater\tpvalue\tfdr\n", fp);
	int rc = 0;
	if (T) {
		uint32_t* pair = (uint32_t*) malloc(T * 2 * sizeof(uint32_t));
		uint8_t* skip = (uint8_t*) malloc(T);
		vdjx_sel_test* out = (vdjx_sel_test*) calloc(T, sizeof(vdjx_sel_test));
		for (size_t r = 0; r < T; r++) {
			pair[2 * r] = (uint32_t) (2 * r + 1); pair[2 * r + 1] = (uint32_t) (2 * r);      /* a = cdr (region 1), b = fwr (region 0) */
			skip[r] = !st[2 * r].sequences || !st[2 * r + 1].sequences;
		}
		rc = vdjx_selection_compare(pdf, 2 * T, pair, T, skip, out);
		if (rc) fprintf(stderr, "--selection-test: %s\n", vdjx_last_error());
		for (size_t r = 0; r < T && !rc; r++) {
			if (skip[r]) fprintf(fp, "%s\t%s\tcdr\tfwr\t\t\t\t\t\n", level[r], id[r]);
			else fprintf(fp, "%s\t%s\tcdr\tfwr\t%.4f\t%.4f\t%.4f\t%.4f\t%.4f\n", level[r], id[r], sel_no_minus_zero(st[2 * r + 1].sigma), sel_no_minus_zero(st[2 * r].sigma),
			             out[r].p_greater, out[r].pvalue, out[r].fdr);
		}
		free(pair); free(skip); free(out);
	}
	if (fclose(fp) && !rc) { fprintf(stderr, "cannot write %s\n", path); return -1; }
	return rc;
}

static int sel_run(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) {
	FILE* fp = fopen(u->c->selection, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->selection); return -1; }
	fputs("level\tid\tregion\tsequences\tobs_r\tobs_s\texp_r\texp_s\tsigma\tsigma_lower\tsigma_upper\tp_positive\n", fp);
	const uint32_t K = u->c->have_regs ? 2 : 1, G = u->c->lineages && n ? u->li.clones : 0;
	int rc = 0, test_refused = 0;
	if (n) {
		const germ_set* g = u->germ;
		int32_t* cdr = NULL;
		if (u->c->have_regs) {
			cdr = (int32_t*) malloc((g->n * 4 + 1) * sizeof(int32_t));
			for (size_t k = 0; k < g->n * 4; k++) cdr[k] = -1;
			const char* first = NULL;
			for (size_t q = 0; q < u->c->nregs; q++) {
				int hit = 0;
				for (size_t r = 0; r < g->n; r++)
					if (!strcmp(g->names[r], u->c->regs[q].name)) { memcpy(cdr + 4 * r, u->c->regs[q].iv, sizeof u->c->regs[q].iv); hit = 1; }
				if (!hit && !u->sel_unmatched++) first = u->c->regs[q].name;
			}
			if (u->sel_unmatched) fprintf(stderr, "--v-regions: %zu names match no germline record (the first: %s)\n", u->sel_unmatched, first);
		}
		int32_t* lim = mutation_limits(ids, contigs, n, len);
		vdjx_sel_counts* cnt = (vdjx_sel_counts*) calloc(n + 1, sizeof(vdjx_sel_counts));
		vdjx_sel_stat* st = (vdjx_sel_stat*) calloc((n + G + 1) * (size_t) K, sizeof(vdjx_sel_stat));
		/* --selection-test: the densities of the lineage and sample rows, and of the consensus sample behind them: T rows of K = 2 */
		const int with_cs = u->c->consensus && u->cs_units;
		const size_t T = (size_t) G + 1 + (with_cs ? 1 : 0);
		int test = u->c->sel_test != NULL;
		if (test && (uint64_t) G + 1 > 65536) {
			fprintf(stderr, "--selection-test: %u lineages (at most 65535): the test table is not written\n", G);
			test = 0; test_refused = 1;
		}
		double* pdf = test ? (double*) malloc(T * K * VDJX_SEL_GRID * sizeof(double)) : NULL;
		vdjx_sel_stat* tst = test ? (vdjx_sel_stat*) calloc(T * K, sizeof(vdjx_sel_stat)) : NULL;
		rc = vdjx_selection(u->gx, contigs, n, len, u->hv, lim, cdr, g->n, u->c->weight, G ? u->lin_clone : NULL, G, cnt, st, u->c->sel_mean ? NULL : pdf, &u->si);
		if (rc) fprintf(stderr, "--selection: %s\n", vdjx_last_error());
		if (!rc && u->c->sel_mean) {
			for (uint32_t k = 0; k < K; k++) u->sel_sigma[k] = sel_no_minus_zero(st[(n + G) * (size_t) K + k].sigma);      /* the selection: line keeps the shared sigma */
			rc = sel_mean_rows(u, cnt, n, K, G ? u->lin_clone : NULL, G, st + n * (size_t) K, pdf);
			for (uint32_t k = 0; k < K && !rc; k++) u->sel_msigma[k] = sel_no_minus_zero(st[(n + G) * (size_t) K + k].sigma);
		}
		if (!rc && test) memcpy(tst, st + n * (size_t) K, ((size_t) G + 1) * K * sizeof(vdjx_sel_stat));
		if (!rc) {
			for (size_t i = 0; i < n; i++) {
				if (cnt[i].flags & 1) sel_rows(fp, "sequence", ids[i], st + i * K, K);
				else fprintf(fp, "sequence\t%s\t\t\t\t\t\t\t\t\t\t\n", ids[i]);
			}
			for (uint32_t k = 0; k < G; k++) {
				char id[32];
				snprintf(id, sizeof id, "lin_%u", k + 1);
				sel_rows(fp, "lineage", id, st + (n + k) * (size_t) K, K);
			}
			sel_rows(fp, "sample", u->c->sample, st + (n + G) * (size_t) K, K);
			/* --consensus: the units' pseudo-contigs, each on its own and all under a shared sigma -- one representative per clone */
			if (u->c->consensus && u->cs_units) {
				const size_t U = u->cs_units;
				vdjx_sel_counts* cnt2 = (vdjx_sel_counts*) calloc(U + 1, sizeof(vdjx_sel_counts));
				vdjx_sel_stat* st2 = (vdjx_sel_stat*) calloc((U + 1) * (size_t) K, sizeof(vdjx_sel_stat));
				double* pdf2 = test ? pdf + ((size_t) G + 1) * K * VDJX_SEL_GRID : NULL;
				rc = vdjx_selection(u->gx, u->cs_pc, U, u->cs_plen, u->cs_hv, NULL, cdr, g->n, u->c->weight, NULL, 0, cnt2, st2, u->c->sel_mean ? NULL : pdf2, NULL);
				if (rc) fprintf(stderr, "--selection: %s\n", vdjx_last_error());
				if (!rc && u->c->sel_mean) rc = sel_mean_rows(u, cnt2, U, K, NULL, 0, st2 + U * (size_t) K, pdf2);
				if (!rc && test) memcpy(tst + ((size_t) G + 1) * K, st2 + U * (size_t) K, K * sizeof(vdjx_sel_stat));
				for (size_t k = 0; k < U && !rc; k++) {
					char id[32];
					snprintf(id, sizeof id, "lin_%d", u->cs_un[k].group + 1);
					const char* name = u->cs_un[k].group >= 0 ? id : ids[u->cs_first[k]];
					if (cnt2[k].flags & 1) sel_rows(fp, "consensus", name, st2 + k * K, K);
					else fprintf(fp, "consensus\t%s\t\t\t\t\t\t\t\t\t\t\n", name);
				}
				if (!rc) sel_rows(fp, "consensus_sample", u->c->sample, st2 + U * (size_t) K, K);
				free(cnt2); free(st2);
			}
			for (uint32_t k = 0; k < K && !u->c->sel_mean; k++) {       /* (mean: kept before the rows were replaced) */
				const double sg = st[(n + G) * (size_t) K + k].sigma;
				u->sel_sigma[k] = sg > -0.00005 && sg < 0.0 ? 0.0 : sg;
			}
		}
		if (!rc && test) {
			const char** level = (const char**) malloc(T * sizeof(char*));
			char** id = (char**) malloc(T * sizeof(char*));
			for (size_t r = 0; r < T; r++) {
				level[r] = r < G ? "lineage" : r == G ? "sample" : "consensus_sample";
				id[r] = (char*) malloc(r < G ? 32 : strlen(u->c->sample) + 1);
				if (r < G) snprintf(id[r], 32, "lin_%zu", r + 1);
				else strcpy(id[r], u->c->sample);
			}
			rc = sel_test_write(u->c->sel_test, level, id, T, tst, pdf);
			for (size_t r = 0; r < T; r++) free(id[r]);
			free(level); free(id);
		}
		free(cdr); free(lim); free(cnt); free(st); free(pdf); free(tst);
	} else if (u->c->sel_test) {
		rc = sel_test_write(u->c->sel_test, NULL, NULL, 0, NULL, NULL);
	}
	u->si.groups = G;
	u->si.regions = K;
	if (fclose(fp) && !rc) { fprintf(stderr, "cannot write %s\n", u->c->selection); return -1; }
	return rc ? rc : test_refused ? -1 : 0;
}

/* --targeting-model: the sample's own 5-mer targeting model (the model: include/vdjx.h, vdjx_targeting_counts and vdjx_targeting_model),
 * in the format --targeting reads: '#' lines with what it was made of, then the 1,024 5-mers in index order.  The limit is --mutations';
 * the lineages of --lineages are the groups, a contig in no lineage is a unit of its own.  --targeting-counts: the counts, a row per 5-mer. */
static int tgt_run(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) {
	static const char B[5] = "ACGT";
	uint64_t* cnt = (uint64_t*) calloc(2 * 2 * 1024 * 4, sizeof(uint64_t));
	uint32_t* w = (uint32_t*) calloc(1024 * 4, sizeof(uint32_t));
	uint8_t* lv = (uint8_t*) calloc(1024 * 2, 1);
	int rc = 0;
	if (n) {
		int32_t* lim = mutation_limits(ids, contigs, n, len);
		rc = vdjx_targeting_counts(u->gx, contigs, n, len, u->hv, lim, u->c->lineages ? u->lin_clone : NULL, cnt, &u->tgi);
		free(lim);
	}
	if (!rc) rc = vdjx_targeting_model(cnt, u->c->tgt_cls, u->c->tgt_min_sub, u->c->tgt_min_mut, w, lv);
	if (rc) fprintf(stderr, "--targeting-model: %s\n", vdjx_last_error());
	if (!rc) {
		for (int m = 0; m < 1024; m++)
			for (int t = 0; t < 2; t++) u->tgt_levels[t][lv[2 * m + t] == 5 ? 0 : lv[2 * m + t] == 3 ? 1 : lv[2 * m + t] == 1 ? 2 : 3]++;
		FILE* fp = fopen(u->c->tgt_model, "w");
		if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->tgt_model); rc = -1; }
		else {
			fprintf(fp, "# targeting model of %s: class %s, min_sub %llu, min_mut %llu\n", u->c->sample, u->c->tgt_cls ? "rs" : "s", (unsigned long long) u->c->tgt_min_sub,
			        (unsigned long long) u->c->tgt_min_mut);
			fprintf(fp, "# %llu units, %llu positions, observed %llu S %llu R, opportunities %llu S %llu R\n", (unsigned long long) u->tgi.units,
			        (unsigned long long) u->tgi.positions, (unsigned long long) u->tgi.obs_s, (unsigned long long) u->tgi.obs_r, (unsigned long long) u->tgi.opp_s,
			        (unsigned long long) u->tgi.opp_r);
			fprintf(fp, "# substitution levels 5/3/1/0: %u/%u/%u/%u 5-mers\n", u->tgt_levels[0][0], u->tgt_levels[0][1], u->tgt_levels[0][2], u->tgt_levels[0][3]);
			fprintf(fp, "# mutability levels 5/3/1/0: %u/%u/%u/%u 5-mers\n", u->tgt_levels[1][0], u->tgt_levels[1][1], u->tgt_levels[1][2], u->tgt_levels[1][3]);
			for (int m = 0; m < 1024; m++)
				fprintf(fp, "%c%c%c%c%c\t%u\t%u\t%u\t%u\n", B[m >> 8 & 3], B[m >> 6 & 3], B[m >> 4 & 3], B[m >> 2 & 3], B[m & 3], w[4 * m], w[4 * m + 1], w[4 * m + 2],
				        w[4 * m + 3]);
			if (fclose(fp)) { fprintf(stderr, "cannot write %s\n", u->c->tgt_model); rc = -1; }
		}
	}
	if (!rc && u->c->tgt_counts) {
		FILE* fp = fopen(u->c->tgt_counts, "w");
		if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->tgt_counts); rc = -1; }
		else {
			fputs("kmer", fp);
			for (int t = 0; t < 4; t++)
				for (int x = 0; x < 4; x++) fprintf(fp, "\t%s_%c_%c", t < 2 ? "obs" : "opp", t & 1 ? 'r' : 's', "acgt"[x]);
			fputs("\tsub_level\tmut_level\n", fp);
			for (int m = 0; m < 1024; m++) {
				fprintf(fp, "%c%c%c%c%c", B[m >> 8 & 3], B[m >> 6 & 3], B[m >> 4 & 3], B[m >> 2 & 3], B[m & 3]);
				for (int t = 0; t < 4; t++)
					for (int x = 0; x < 4; x++) fprintf(fp, "\t%llu", (unsigned long long) cnt[(size_t) t * 4096 + 4 * (size_t) m + (size_t) x]);
				fprintf(fp, "\t%u\t%u\n", lv[2 * m], lv[2 * m + 1]);
			}
			if (fclose(fp)) { fprintf(stderr, "cannot write %s\n", u->c->tgt_counts); rc = -1; }
		}
	}
	free(cnt); free(w); free(lv);
	return rc;
}

/* --consensus: the consensus V sequence of every unit (the model: include/vdjx.h, vdjx_consensus): the lineages of --lineages are the
 * groups, a contig in no lineage is a unit of its own, the limit is --mutations'.  A row per unit, in unit order; the six mutation cells are
 * vdjx_mutations' counts of the unit's pseudo-contig under its synthetic hit (vdjx_consensus_hits), J absent, no limit.  The pseudo-contigs
 * are kept for the --selection table's consensus rows. */
static int cons_run(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) {
	FILE* fp = fopen(u->c->consensus, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->consensus); return -1; }
	fputs("clone_id\tsequence_id\tv_call\tmembers\toff_record\tgermline_start\tgermline_end\tconsensus_alignment\tgermline_alignment\tmin_cover\tundecided\t"
	      "v_germline_codons\tmu_count_v_r\tmu_count_v_s\tmu_count_v_stop\tmu_count_v_na\tmu_freq_v\n", fp);
	int rc = 0;
	if (n) {
		const germ_set* g = u->germ;
		int32_t* lim = mutation_limits(ids, contigs, n, len);
		int32_t* unit = (int32_t*) calloc(n + 1, sizeof(int32_t));
		vdjx_cons_unit* un = (vdjx_cons_unit*) calloc(n + 1, sizeof(vdjx_cons_unit));
		uint64_t U = 0, cols = 0;
		char *cons = NULL, *germ = NULL;
		uint32_t* cover = NULL;
		vdjx_mut_row* rows = NULL;
		vdjx_annot_hit* nohit = NULL;
		rc = vdjx_consensus_layout(u->hv, lim, u->lin_clone, n, len, unit, un, &U, &cols);
		if (!rc) {
			cons = (char*) malloc((size_t) cols + 1);
			germ = (char*) malloc((size_t) cols + 1);
			cover = (uint32_t*) calloc((size_t) cols + 1, sizeof(uint32_t));
			const vdjx_cons_params cp = {u->c->cons_num, 10000};
			rc = vdjx_consensus(u->gx, contigs, n, len, u->hv, lim, u->lin_clone, &cp, cons, germ, cover, NULL, un, unit, &u->ci);
		}
		int plen = 1;
		if (!rc) rc = vdjx_consensus_hits(un, (size_t) U, cons, germ, 0, NULL, NULL, &plen);
		if (!rc) {
			u->cs_pc = (char*) malloc((size_t) U * (size_t) plen + 1);
			u->cs_hv = (vdjx_annot_hit*) calloc((size_t) U + 1, sizeof(vdjx_annot_hit));
			rc = vdjx_consensus_hits(un, (size_t) U, cons, germ, plen, u->cs_pc, u->cs_hv, &plen);
		}
		rows = (vdjx_mut_row*) calloc((size_t) U + 1, sizeof(vdjx_mut_row));
		if (!rc && U) {
			nohit = (vdjx_annot_hit*) calloc((size_t) U + 1, sizeof(vdjx_annot_hit));
			for (size_t k = 0; k < U; k++) nohit[k].gene = -1;
			rc = vdjx_mutations(u->gx, u->cs_pc, (size_t) U, plen, u->cs_hv, NULL, nohit, NULL, NULL, NULL, NULL, rows, NULL);
		}
		if (rc) fprintf(stderr, "--consensus: %s\n", vdjx_last_error());
		if (!rc) {
			u->cs_units = (size_t) U;
			u->cs_plen = plen;
			u->cs_un = un;
			u->cs_first = (size_t*) calloc((size_t) U + 1, sizeof(size_t));
			for (size_t i = n; i-- > 0;)
				if (unit[i] >= 0) u->cs_first[unit[i]] = i;
			for (size_t k = 0; k < U; k++) {
				const vdjx_cons_unit* q = un + k;
				const int w = q->hi - q->lo;
				uint32_t minc = w ? UINT32_MAX : 0, und = 0;
				for (int x = 0; x < w; x++) {
					const uint32_t cv = cover[q->off + (uint64_t) x];
					if (cv < minc) minc = cv;
					und += cons[q->off + (uint64_t) x] == 'N' && cv > 0;
				}
				if (q->members > u->cs_largest) u->cs_largest = q->members;
				if (q->group >= 0) fprintf(fp, "lin_%d", q->group + 1);
				fprintf(fp, "\t%s\t%s\t%u\t%u\t%d\t%d\t%.*s\t%.*s\t%u\t%u\t", ids[u->cs_first[k]], g->names[q->gene], q->members, q->off_record, q->lo + 1, q->hi, w,
				        cons + q->off, w, germ + q->off, minc, und);
				const vdjx_mut_row* r = rows + k;
				if (r->flags & 1) {
					fprintf(fp, "%d\t%d\t%d\t%d\t%d\t", r->v_codons, r->v_r, r->v_s, r->v_stop, r->v_na);
					if (r->v_codons) fprintf(fp, "%.4f", (double) (r->v_r + r->v_s) / (double) (3 * r->v_codons));
				} else fputs("\t\t\t\t\t", fp);
				fputc('\n', fp);
			}
		} else free(un);
		free(lim); free(unit); free(cons); free(germ); free(cover); free(rows); free(nohit);
	}
	if (fclose(fp) && !rc) { fprintf(stderr, "cannot write %s\n", u->c->consensus); return -1; }
	return rc;
}

/* --diversity: the Hill diversity curve of the lineages (the model: include/vdjx.h, vdjx_diversity; the weights: diversity_weights of
 * vdjer_amd/annot.py).  A lineage's weight is the sum of its members' expected_count as printed, in hundredths, read from the digits;
 * lineages of weight 0 take no part.  A row per order 0.0 .. 4.0: the unresampled value, the replicates' mean and sd, the 95 % normal
 * interval (alakazam's alphaDiversity) and the three over d at q = 0 (evenness).  No lineage of weight: the header alone, no device call. */
#define DIV_ORDERS 41
static int diversity_run(hook_ud* u, size_t n) {
	FILE* fp = fopen(u->c->diversity, "w");
	if (!fp) { fprintf(stderr, "cannot write %s\n", u->c->diversity); return -1; }
	fputs("q\td_observed\td\td_sd\td_lower\td_upper\te\te_lower\te_upper\n", fp);
	const size_t nk = u->li.clones;
	uint64_t* w = (uint64_t*) calloc(nk + 1, sizeof(uint64_t));
	for (size_t i = 0; i < n; i++) {
		if (u->lin_clone[i] < 0) continue;
		char cnt[64];
		snprintf(cnt, sizeof cnt, "%.2f", u->qcnt ? u->qcnt[i] : 0.0);
		uint64_t h = 0;
		for (const char* p = cnt; *p; p++)
			if (*p >= '0' && *p <= '9') h = h * 10 + (uint64_t) (*p - '0');
		w[u->lin_clone[i]] += h;
	}
	size_t C = 0;
	uint64_t W = 0;
	for (size_t k = 0; k < nk; k++)
		if (w[k]) { W += w[k]; w[C++] = w[k]; }
	u->dv_weight = W;
	int rc = 0;
	if (!u->dv_depth) {                    /* the default depth: the total expected pairs rounded half up, at least 1 */
		const uint64_t pairs = (W + 50) / 100;
		if (pairs > 2147483647u) { fprintf(stderr, "--diversity: %llu expected pairs are more than a replicate's 2147483647 draws: give --diversity-depth <n>\n", (unsigned long long) pairs); rc = -1; }
		else u->dv_depth = pairs ? (uint32_t) pairs : 1;
	}
	if (!rc && C) {
		double q[DIV_ORDERS], obs[DIV_ORDERS], mean[DIV_ORDERS], sd[DIV_ORDERS];
		double* d = (double*) calloc((size_t) u->c->div_boot * DIV_ORDERS, sizeof(double));
		for (int k = 0; k < DIV_ORDERS; k++) q[k] = (double) k / 10.0;
		const vdjx_diversity_params dp = {u->c->div_boot, u->dv_depth, u->c->div_seed};
		rc = vdjx_diversity(u->gx, w, C, q, DIV_ORDERS, &dp, obs, d, mean, sd, NULL, &u->dvi);
		if (rc) fprintf(stderr, "--diversity: %s\n", vdjx_last_error());
		if (!rc) {
			const double z = 1.959963984540054, d0 = mean[0];
			for (int k = 0; k < DIV_ORDERS; k++) {
				const double lo = mean[k] - z * sd[k] > 0.0 ? mean[k] - z * sd[k] : 0.0, hi = mean[k] + z * sd[k];
				fprintf(fp, "%.1f\t%.4f\t%.4f\t%.4f\t%.4f\t%.4f\t%.4f\t%.4f\t%.4f\n", q[k], obs[k], mean[k], sd[k], lo, hi, mean[k] / d0, lo / d0, hi / d0);
			}
			u->dv_d0 = mean[0]; u->dv_d1 = mean[10]; u->dv_d2 = mean[20];
		}
		free(d);
	}
	u->dvi.clones = (uint32_t) C;          /* (no lineage of weight: the device was not called) */
	free(w);
	if (fclose(fp) && !rc) { fprintf(stderr, "cannot write %s\n", u->c->diversity); return -1; }
	return rc;
}

/* the tables after the SAM body: every device step runs once, whichever tables ask for it */
static int tables(hook_ud* u, const char* const* ids, const char* contigs, size_t n, int len) {
	int rc = 0;
	if (!rc && (u->c->quant || u->c->clones)) rc = quant_table(u, ids, contigs, n, len);
	if (!rc && (u->c->airr || u->c->clones || u->c->lineages || u->c->mutations || u->c->selection || u->c->tgt_model)) rc = annot_run(u, contigs, n, len);
	if (!rc && u->c->d_calls) rc = dcall_run(u, contigs, n, len);
	if (!rc && u->c->lineages) rc = lineage_run(u, ids, contigs, n, len);
	if (!rc && u->c->trees) rc = tree_run(u, ids, contigs, n, len);
	if (!rc && u->c->trees_nj) rc = tree_nj_run(u, ids, contigs, n, len);
	if (!rc && u->c->trees_mp) rc = tree_mp_run(u, ids, contigs, n, len);
	if (!rc && u->c->diversity) rc = diversity_run(u, n);
	if (!rc && u->c->mutations) rc = mut_run(u, ids, contigs, n, len);
	if (!rc && u->c->consensus) rc = cons_run(u, ids, contigs, n, len);
	if (!rc && u->c->selection) rc = sel_run(u, ids, contigs, n, len);
	if (!rc && u->c->tgt_model) rc = tgt_run(u, ids, contigs, n, len);
	if (!rc && u->c->airr) rc = airr_table(u, ids, contigs, n, len);
	if (!rc && u->c->cfa && (u->c->isotypes || u->c->clones)) rc = iso_run(u, contigs, n, len);
	if (!rc && u->c->isotypes) rc = isotypes_table(u, ids, n, len);
	if (!rc && u->c->clones) rc = clones_table(u, ids, contigs, n, len);
	return rc;
}

static int h_sam_body(void* ud, const char* const* ids, const char* contigs, size_t n, int len, FILE* out) {
	hook_ud* u = (hook_ud*) ud;
	int rc = sam_records(ud, ids, contigs, n, len, out);
	if (!rc) rc = tables(u, ids, contigs, n, len);
	if (!rc) u->tables_ran = 1;
	return rc;
}

/* a line per table on stderr, behind FINIS */
static void tables_summary(const hook_ud* u) {
	const cli* c = u->c;
	if (c->quant)
		fprintf(stderr, "quant: %llu pairs placed (%llu once), %llu alignments, %u EM iterations, %s; table in %s\n", (unsigned long long) u->qi.pairs,
		        (unsigned long long) u->qi.unique_pairs, (unsigned long long) u->qi.alignments, u->qi.iterations,
		        u->qi.converged ? "converged" : "stopped at the iteration limit", c->quant);
	if (c->quant && c->qb_b)
		fprintf(stderr, "quant boot: %u replicates (seed %llu), %llu EM iterations in all (most %u), %u stopped at the iteration limit, %u batches\n", u->qbi.replicates,
		        (unsigned long long) c->qb_seed, (unsigned long long) u->qbi.iterations, u->qbi.max_iterations, u->qbi.replicates - u->qbi.converged, u->qbi.batches);
	if (c->airr)
		fprintf(stderr, "airr: %zu contigs, %zu V called, %zu J called, %zu productive, %zu CIGARs truncated; germline records skipped: %zu D, %zu other; table in %s\n",
		        u->a_contigs, u->a_v, u->a_j, u->a_prod, u->a_trunc, u->a_skip_d, u->a_skip_other, c->airr);
	if (c->d_calls)
		fprintf(stderr, "dcalls: %zu contigs, %zu windows, %zu over %d bases, %zu D called against %zu D records\n", u->d_contigs, u->d_windows, u->d_over,
		        VDJX_DCALL_WINDOW, u->d_called, u->dset ? u->dset->n : (size_t) 0);
	if (c->lineages)
		fprintf(stderr, "lineages: %zu contigs, %zu eligible, %u buckets (largest %u), %llu pairs, %llu links, %u lineages at %d/%d\n", u->l_contigs, u->l_eligible,
		        u->li.buckets, u->li.largest_bucket, (unsigned long long) u->li.pairs, (unsigned long long) u->li.links, u->li.clones, u->lin_num, c->lin_den);
	if (c->lin_model)
		fprintf(stderr, "lineage model: %s, symmetry %s, mean %.4f, costs %u .. %u, %llu of %llu ordered pairs walked\n", c->lin_model, c->lin_sym ? "min" : "avg",
		        c->lin_ti.mean, c->lin_ti.min_cost, c->lin_ti.max_cost, u->lin_walked, 2ull * (unsigned long long) u->li.pairs);
	if (c->lin_threshold) {
		static const char* const why[5] = {"", "too few values", "no scale", "one mode", "shallow valley"};
		const vdjx_threshold_info* t = &u->thi;
		if (t->status == VDJX_THRESHOLD_FOUND)
			fprintf(stderr, "lineage threshold: %u distances in %u bins, bandwidth %.3f, peaks %.4f %.4f, valley %.4f .. %.4f, threshold %.4f, %d pair passes\n", t->values,
			        t->distinct, t->k / 1000.0, t->p1_first / 10000.0, t->p2_first / 10000.0, t->t_first / 10000.0, t->t_last / 10000.0, t->threshold / 10000.0, u->thr_passes);
		else
			fprintf(stderr, "lineage threshold: %u distances in %u bins, none (%s), --lineage-dist %.4f stands\n", t->values, t->distinct, why[t->status <= 4 ? t->status : 0],
			        u->thr_fallback / 10000.0);
	}
	if (c->lin_linkage)
		fprintf(stderr, "lineage link: %s, %u components of two and more (largest %u), %u merges, %u lineages of %u under single linkage, %u batches\n", c->lin_linkage == 1 ? "complete" : "average",
		        u->lki.components, u->lki.largest_component, u->lki.merges, u->li.clones, u->lki.clones_single, u->lki.batches);
	if (c->trees)
		fprintf(stderr, "trees: %u contigs in %u lineages (largest %u), %llu edges, total distance %llu, %u rounds\n", u->ti.members, u->ti.clones, u->ti.largest_clone,
		        (unsigned long long) u->ti.edges, (unsigned long long) u->ti.weight, u->ti.rounds);
	if (c->ts_b)
		fprintf(stderr, "tree support: %u replicates (seed %llu), %llu edges, %llu of %llu kept, %llu in every replicate, %u batches\n", c->ts_b,
		        (unsigned long long) c->ts_seed, (unsigned long long) u->tsi.edges, (unsigned long long) u->tsi.matched,
		        (unsigned long long) (u->tsi.edges * c->ts_b), (unsigned long long) u->tsi.full, u->tsi.batches);
	if (c->trees_nj)
		fprintf(stderr, "trees nj: %u contigs in %u lineages (largest %u), %u inferred nodes, %llu edges, length %.4f, parsimony %llu, %u negative branches, %u batches\n",
		        u->tni.members, u->tni.clones, u->tni.largest_clone, u->tni.internal, (unsigned long long) u->tni.edges, (double) u->tni.length / 65536.0,
		        (unsigned long long) u->tni.parsimony, u->tni.negative, u->tni.batches);
	if (c->trees_mp)
		fprintf(stderr, "trees mp: %u contigs in %u lineages (largest %u), %u searched, %u improved, %llu moves in %u rounds, %llu candidates, parsimony %llu -> %llu, %u batches\n",
		        u->tmi.members, u->tmi.clones, u->tmi.largest_clone, u->tmi.searched, u->tmi.moved, (unsigned long long) u->tmi.moves, u->tmi.rounds,
		        (unsigned long long) u->tmi.candidates, (unsigned long long) u->tmi.parsimony_start, (unsigned long long) u->tmi.parsimony, u->tmi.batches);
	if (c->isotypes)
		fprintf(stderr, "isotypes: %zu contigs, %zu called against %zu constant records of %s; table in %s\n", u->i_contigs, u->i_called,
		        u->cst ? u->cst->n : (size_t) 0, c->cfa, c->isotypes);
	if (c->clones)
		fprintf(stderr, "clones: %zu rows in %zu clusters, isotypes %s; table in %s\n", u->c_rows, u->c_clusters, c->cfa ? "called" : "N/A (no --cfa)", c->clones);
	if (c->mutations)
		fprintf(stderr, "mutations: %llu contigs, %llu aligned, %llu columns, %llu V codons, %llu R, %llu S, %llu stop, %llu unclassified, %u J clipped, %u over 64 runs\n",
		        (unsigned long long) u->mi.contigs, (unsigned long long) u->mi.aligned, (unsigned long long) u->mi.cols, (unsigned long long) u->mi.v_codons,
		        (unsigned long long) u->mi.v_r, (unsigned long long) u->mi.v_s, (unsigned long long) u->mi.v_stop, (unsigned long long) u->mi.v_na,
		        u->mi.clipped, u->mi.truncated);
	if (c->diversity)
		fprintf(stderr, "diversity: %u lineages with weight of %u, %llu.%02llu expected pairs, depth %u, %u replicates (seed %llu), richness %.2f, shannon %.4f, simpson %.4f, %u batches\n",
		        u->dvi.clones, u->li.clones, (unsigned long long) (u->dv_weight / 100), (unsigned long long) (u->dv_weight % 100), u->dv_depth, c->div_boot,
		        (unsigned long long) c->div_seed, u->dv_d0, u->dv_d1, u->dv_d2, u->dvi.batches);
	if (c->selection) {
		fprintf(stderr, "selection: %llu contigs, %llu used, %llu without regions, %u lineages, %u regions, targeting %s, sample sigma %.4f", (unsigned long long) u->si.contigs,
		        (unsigned long long) u->si.used, (unsigned long long) u->si.no_regions, u->si.groups, u->si.regions, c->targeting ? c->targeting : "uniform", u->sel_sigma[0]);
		if (u->si.regions == 2) fprintf(stderr, " %.4f", u->sel_sigma[1]);
		fprintf(stderr, ", %u chunks\n", u->si.chunks);
		if (c->sel_mean) {
			fprintf(stderr, "selection combine: mean, %u rows, %llu densities, %llu combinations, %u levels at most, %u batches, sample sigma %.4f", u->sci.rows,
			        (unsigned long long) u->sci.leaves, (unsigned long long) u->sci.combines, u->sci.levels, u->sci.batches, u->sel_msigma[0]);
			if (u->si.regions == 2) fprintf(stderr, " %.4f", u->sel_msigma[1]);
			fputc('\n', stderr);
		}
	}
	if (c->tgt_model)
		fprintf(stderr, "targeting model: %llu contigs, %llu used, %llu units, %llu positions, %llu S, %llu R, class %s, substitution levels %u/%u/%u/%u, mutability levels %u/%u/%u/%u, %u batches\n",
		        (unsigned long long) u->tgi.contigs, (unsigned long long) u->tgi.used, (unsigned long long) u->tgi.units, (unsigned long long) u->tgi.positions,
		        (unsigned long long) u->tgi.obs_s, (unsigned long long) u->tgi.obs_r, c->tgt_cls ? "rs" : "s", u->tgt_levels[0][0], u->tgt_levels[0][1], u->tgt_levels[0][2],
		        u->tgt_levels[0][3], u->tgt_levels[1][0], u->tgt_levels[1][1], u->tgt_levels[1][2], u->tgt_levels[1][3], u->tgi.batches);
	if (c->consensus)
		fprintf(stderr, "consensus: %llu contigs, %llu used, %llu units (largest %u), %llu off the unit's record, %llu columns, %llu undecided, min share %d.%04d, %u batches\n",
		        (unsigned long long) u->ci.contigs, (unsigned long long) u->ci.used, (unsigned long long) u->ci.units, u->cs_largest, (unsigned long long) u->ci.off_record,
		        (unsigned long long) u->ci.columns, (unsigned long long) u->ci.undecided, c->cons_num / 10000, c->cons_num % 10000, u->ci.batches);
}

static void h_status(void* ud, const char* desc) { (void) ud; status(desc); }

#define VX(call) do { if ((call) != 0) { fprintf(stderr, "%s: %s\n", #call, vdjx_last_error()); return 1; } } while (0)

/* ---- `--gpus N`: the other ranks are child processes.  A rank that fails must never leave the others waiting inside a collective
 * (RCCL has no timeout of its own): a child dies with its parent (PR_SET_PDEATHSIG), the parent takes every child down when it
 * leaves for whatever reason (atexit), and a child that ends badly ends the whole run at once (SIGCHLD) instead of hanging it. */
static pid_t g_kids[256];
static volatile sig_atomic_t g_kid_state[256];      /* 0 running, 1 ended well, 2 reaped after being killed */
static int g_nkids = 0;

static volatile sig_atomic_t g_leaving = 0;       /* the parent is taking the ranks down itself: their end is not a failure to report */

static void kill_kids(void) {
	/* a deliberate teardown (rank 0 failed on its own, or is done): no SIGCHLD handler run from here on, so the exit status the
	 * caller chose survives and nobody blames a GPU rank for a host-side error */
	sigset_t chld;
	sigemptyset(&chld);
	sigaddset(&chld, SIGCHLD);
	sigprocmask(SIG_BLOCK, &chld, NULL);
	g_leaving = 1;
	for (int r = 1; r <= g_nkids; r++) if (g_kid_state[r] == 0) (void) kill(g_kids[r], SIGTERM);
	for (int r = 1; r <= g_nkids; r++) if (g_kid_state[r] == 0) { int st_; (void) waitpid(g_kids[r], &st_, 0); g_kid_state[r] = 2; }
}

static void on_sigchld(int sig) {
	(void) sig;
	if (g_leaving) return;
	for (int r = 1; r <= g_nkids; r++) {
		if (g_kid_state[r] != 0) continue;
		int st_ = 0;
		const pid_t p = waitpid(g_kids[r], &st_, WNOHANG);
		if (p != g_kids[r]) continue;
		if (WIFEXITED(st_) && WEXITSTATUS(st_) == 0) { g_kid_state[r] = 1; continue; }
		g_kid_state[r] = 2;
		static const char msg[] = "vdjer: a GPU rank failed; stopping the others\n";
		(void) !write(2, msg, sizeof msg - 1);
		for (int q = 1; q <= g_nkids; q++) if (g_kid_state[q] == 0) (void) kill(g_kids[q], SIGKILL);
		for (int q = 1; q <= g_nkids; q++) if (g_kid_state[q] == 0) { int s2; (void) waitpid(g_kids[q], &s2, 0); }      /* (no zombies left to whoever inherits them) */
		_exit(1);
	}
}

static void report_share(int rank, const reads_t* rd) {
	if (!vdjx_env_set("VDJX_REPORT_SHARE")) return;
	struct rusage ru;
	getrusage(RUSAGE_SELF, &ru);
	fprintf(stderr, "share\trank\t%d\trecords\t%zu\tof\t%llu\tpairs\t%u\thost_pool_bytes\t%zu\tmaxrss_kb\t%ld\n", rank, rd->n_primary + rd->n_secondary,
	        (unsigned long long) rd->total_records, rd->n_pairs, (rd->n_primary + rd->n_secondary) * (2 * (size_t) rd->rl + 1), ru.ru_maxrss);
}

int main(int argc, char** argv) {
	t_start = t_prev = time(NULL);
	g_times = vdjx_times();
	cli c;
	if (parse(argc, argv, &c)) return 255;                  /* the reference exits with -1 */
	/* --gpus N: one process per GPU.  The parent is rank 0; ranks 1..N-1 are forked BEFORE anything touches a GPU.  Every rank reads
	 * the input and keeps ITS share of the pool (the pairs whose name hashes to it), the ranks deal the k-mer build's slices out to
	 * each other on the devices, build the graph together, and the others then serve rank 0's scorer calls (vdjx_mgpu.h) while it
	 * runs the serial traversal. */
	const char* dump_share = vdjx_env_str("VDJX_DUMP_SHARE");
	if (dump_share) {            /* (test hook, no GPU: "rank,nranks" -> that rank's share: its records on stdout, their places on stderr) */
		int rk = 0, nr = 1;
		reads_t sh;
		if (sscanf(dump_share, "%d,%d", &rk, &nr) != 2 || nr < 1 || rk < 0 || rk >= nr || load_reads(&c, &sh, rk, nr, nr > 1)) return 255;
		const size_t R = sh.n_primary + sh.n_secondary;
		fprintf(stderr, "share\t%d\t%d\trl\t%d\trecords\t%zu\ttotal\t%llu\tpairs\t%u\n", rk, nr, sh.rl, R, (unsigned long long) sh.total_records, sh.n_pairs);
		for (size_t i = 0; i < R; i++) fprintf(stderr, "rec\t%u\t%u\t%u\t%d\t%d\t%s\n", sh.scan_index[i], sh.reg_rank[i], sh.pair_id[i], sh.read_num[i], sh.is_rc[i], sh.names[sh.pair_id[i]]);
		fwrite(sh.primary, 2 * (size_t) sh.rl + 1, sh.n_primary, stdout);
		if (sh.n_secondary) fwrite(sh.secondary, 2 * (size_t) sh.rl + 1, sh.n_secondary, stdout);
		return 0;
	}
	int rank = 0;
	if (c.gpus < 1 || c.gpus > 256) { fprintf(stderr, "--gpus must be in [1,256]\n"); return 255; }
	const int use_mgpu = c.gpus > 1 || vdjx_env_set("VDJX_FORCE_MGPU");      /* (the variable: a one-rank run of the same code path) */
	if (c.quant && use_mgpu) {
		fprintf(stderr, "--quant runs on one GPU only: it cannot be combined with --gpus N > 1 (or VDJX_FORCE_MGPU)\n");
		return 255;
	}
	if (c.clones && use_mgpu) {
		fprintf(stderr, "--clones runs on one GPU only (its counts are --quant's): it cannot be combined with --gpus N > 1 (or VDJX_FORCE_MGPU)\n");
		return 255;
	}
	/* ranks that share ONE device (the multi-rank tests on a one-GPU box; RCCL refuses two ranks on a device): bytes move through the
	 * host.  Otherwise rank r drives GPU r and the bytes move by RCCL over xGMI. */
	const int one_device = vdjx_env_set("VDJX_MGPU_ONE_DEVICE");
	const char* transport = one_device ? "host" : (vdjx_env_str("VDJX_MGPU_TRANSPORT") ? vdjx_env_str("VDJX_MGPU_TRANSPORT") : "rccl");
	int* fds = NULL;
	if (c.gpus > 1) {
		fds = (int*) malloc((size_t) c.gpus * (size_t) c.gpus * sizeof(int));
		if (vdjx_comm_sockets(c.gpus, !strcmp(transport, "host"), fds)) { fprintf(stderr, "%s\n", vdjx_comm_last_error()); return 255; }
		struct sigaction sa;
		memset(&sa, 0, sizeof sa);
		sa.sa_handler = on_sigchld;
		sa.sa_flags = SA_RESTART | SA_NOCLDSTOP;
		sigaction(SIGCHLD, &sa, NULL);
		atexit(kill_kids);
	}
	const pid_t parent = getpid();
	sigset_t chld, before;
	sigemptyset(&chld);
	sigaddset(&chld, SIGCHLD);
	sigprocmask(SIG_BLOCK, &chld, &before);       /* (no rank's end is handled before every rank is on the list) */
	for (int r = 1; r < c.gpus; r++) {
		fflush(stdout); fflush(stderr);
		const pid_t pid = fork();
		if (pid < 0) { perror("fork"); return 255; }
		if (pid == 0) {
			rank = r; g_rank = r; g_nkids = 0;
			signal(SIGCHLD, SIG_DFL);
			sigprocmask(SIG_SETMASK, &before, NULL);
			(void) prctl(PR_SET_PDEATHSIG, SIGKILL);
			if (getppid() != parent) _exit(1);             /* (the parent was gone before the request took effect) */
			break;
		}
		g_kids[r] = pid;
		g_nkids = r;
	}
	if (fds) vdjx_comm_sockets_keep(c.gpus, rank, fds);
	if (rank == 0) sigprocmask(SIG_SETMASK, &before, NULL);
	if (rank == 0) status("START");
	/* the GPU context starts on a thread of its own while this one reads the input: bringing up the HIP runtime takes a few hundred
	 * milliseconds, about what parsing a few hundred thousand pairs takes.  (After the forks: no rank touches a GPU before it is a
	 * process of its own, and nothing is ever exec'ed from here.) */
	const int device = one_device ? 0 : rank;              /* rank r drives GPU r */
	init_job ij;
	memset(&ij, 0, sizeof ij);
	ij.device = device;
	pthread_t init_th;
	const int init_threaded = pthread_create(&init_th, NULL, init_thread, &ij) == 0;
	reads_t rd;
	/* an input error between here and the join below must not run exit() and its handlers while the HIP runtime is still coming up on the
	 * other thread: wait for that thread, then leave with the documented code */
#define BAIL(code) do { if (init_threaded) pthread_join(init_th, NULL); return (code); } while (0)
	if (load_reads(&c, &rd, rank, c.gpus, use_mgpu)) BAIL(255);
	c.hp.read_length = rd.rl;
	c.hp.threads = c.threads;
	if (rank == 0) fprintf(stderr, "read length:\t%d\n", rd.rl);

	uint32_t *vc = NULL, *jc = NULL;
	size_t nv = 0, nj = 0;
	if (load_codes(c.v_anchors, c.anchor_mismatches, &vc, &nv) || load_codes(c.j_anchors, c.anchor_mismatches, &jc, &nj)) BAIL(255);
	qsort(vc, nv, 4, cmp_u32);
	qsort(jc, nj, 4, cmp_u32);
	char** vlines = NULL;
	size_t nvl = 0;
	if (load_vregion(c.source_sim_file, &vlines, &nvl)) BAIL(255);
#undef BAIL

	vdjx_ctx* gx = NULL;
	if (g_times) status("(inputs read)");
	if (init_threaded) pthread_join(init_th, NULL);
	else init_thread(&ij);
	if (ij.rc) { fprintf(stderr, "vdjx_init: %s\n", ij.err); return 1; }
	gx = ij.gx;
	if (g_times) status("(vdjx_init done)");
	vdjx_mgpu* mg = NULL;
	if (use_mgpu) {
		unsigned char id[VDJX_COMM_ID_BYTES];
		memset(id, 0, sizeof id);
		/* the communicator's bootstrap id: made by rank 0 (RCCL only; zeros otherwise), handed to every rank over its control socket --
		 * whatever the transport, so that the hand-over itself runs in the one-device tests too */
		const int* my_fds = fds ? fds + (size_t) rank * (size_t) c.gpus : NULL;
		if (rank == 0) {
			if (!strcmp(transport, "rccl") && vdjx_comm_unique_id(id)) { fprintf(stderr, "%s\n", vdjx_comm_last_error()); return 1; }
			for (int r = 1; r < c.gpus; r++)
				for (size_t at = 0; at < sizeof id;) {
					const ssize_t k = write(my_fds[r], id + at, sizeof id - at);
					if (k <= 0) { if (k < 0 && errno == EINTR) continue; perror("write"); return 1; }
					at += (size_t) k;
				}
		} else {
			for (size_t at = 0; at < sizeof id;) {
				const ssize_t k = read(my_fds[0], id + at, sizeof id - at);
				if (k <= 0) { if (k < 0 && errno == EINTR) continue; fprintf(stderr, "rank %d: no communicator id from rank 0\n", rank); return 1; }
				at += (size_t) k;
			}
		}
		vdjx_comm* cm = NULL;
		if (vdjx_comm_init(transport, rank, c.gpus, device, my_fds, id, &cm)) { fprintf(stderr, "rank %d: %s\n", rank, vdjx_comm_last_error()); return 1; }
		if (vdjx_mgpu_init(cm, device, &mg)) { fprintf(stderr, "rank %d: %s\n", rank, vdjx_mgpu_last_error()); return 1; }
	}
	VX(vdjx_anchor_sets_load(gx, vc, nv, jc, nj));
	VX(vdjx_vregion_load(gx, (const char* const*) vlines, nvl, c.hp.vregion_kmer_size));
	status("POST_VJF_INIT");

	vdjx_pool* px = NULL;
	if (!use_mgpu) {
		VX(vdjx_pool_load(gx, rd.primary, rd.n_primary, rd.secondary, rd.n_secondary, rd.rl, &px));
		if (g_times) status("(pool loaded)");
		/* the read index (add_read_info, quick_map3.c:126-149) is begun on the library's index stream and built BESIDE the k-mer build below:
		 * both only read the packed pool, and nothing needs the index before the traversal's first window (A2:841).  It is ended after
		 * the build */
		VX(vdjx_read_index_build_begin(gx, px, rd.pair_id, rd.read_num, rd.is_rc, rd.reg_rank, rd.n_pairs));
		if (g_times) status("(read index begun)");
	} else if (vdjx_mgpu_load(mg, gx, rd.primary, rd.n_primary, rd.rl, rd.scan_index, rd.pair_id, rd.read_num, rd.is_rc, rd.reg_rank, rd.n_pairs, rd.total_records)) {
		fprintf(stderr, "%s\n", vdjx_mgpu_last_error());
		return 1;
	}
	if (vdjx_stat(gx, "pool_other_bases"))
		fprintf(stderr, "warning: %llu bases other than ACGTN in the reads%s are treated as N (the reference would carry them inside k-mers)\n",
		        (unsigned long long) vdjx_stat(gx, "pool_other_bases"), use_mgpu ? " of this rank" : "");
	{	/* the read names by pair id, for the SAM records formatted on the device */
		uint64_t* noff = (uint64_t*) calloc((size_t) rd.n_pairs + 1, 8);
		for (uint32_t i = 0; i < rd.n_pairs; i++) noff[i + 1] = noff[i] + strlen(rd.names[i]);
		char* cat = (char*) malloc((size_t) noff[rd.n_pairs] + 1);
		for (uint32_t i = 0; i < rd.n_pairs; i++) memcpy(cat + noff[i], rd.names[i], (size_t) (noff[i + 1] - noff[i]));
		const int rcn = vdjx_sam_names_load(gx, cat, noff, rd.n_pairs);
		free(cat);
		free(noff);
		if (rcn) { fprintf(stderr, "vdjx_sam_names_load: %s\n", vdjx_last_error()); return 1; }
	}
	report_share(rank, &rd);
	if (use_mgpu) {                              /* the records live on the device now (the share's quality characters included) */
		free(rd.primary); rd.primary = NULL;
		free(rd.pair_id); free(rd.reg_rank); free(rd.scan_index); free(rd.read_num); free(rd.is_rc);
		rd.pair_id = rd.reg_rank = rd.scan_index = NULL; rd.read_num = rd.is_rc = NULL;
	}
	status("POST_READ_EXTRACT");
	if (rank == 0) fprintf(stderr, "Assembling...\n");
	vdjx_graph* gg = NULL;
	status("PRE_PRE_GRAPH1");                  /* A2:1387 */
	if (!use_mgpu) {
		VX(vdjx_kmer_build(gx, px, c.hp.k, c.hp.min_node_freq, c.hp.min_base_quality, &gg));
		if (g_times) status("(k-mer build done)");
		VX(vdjx_read_index_build_end(gx));
		if (g_times) status("(read index ended)");
	} else {
		if (vdjx_mgpu_kmer_build(mg, gx, c.hp.k, c.hp.min_node_freq, c.hp.min_base_quality, &gg)) { fprintf(stderr, "%s\n", vdjx_mgpu_last_error()); return 1; }
		if (rank == 0) fprintf(stderr, "k-mer table sharded over %d GPUs (%s): %llu bytes sent by rank 0 so far\n", c.gpus, transport, (unsigned long long) vdjx_mgpu_bytes_sent(mg));
		if (rank != 0) {                        /* the graph is identical on every rank; the serial traversal runs on rank 0, which calls on the others' scorers */
			vdjx_graph_free(gg);
			const int rcs = vdjx_mgpu_serve(mg, gx);
			if (rcs) fprintf(stderr, "%s\n", vdjx_mgpu_last_error());
			vdjx_mgpu_free(mg);
			vdjx_shutdown(gx);
			return rcs ? 1 : 0;
		}
	}
	const size_t n = vdjx_graph_nodes(gg);
	status("PRE_PRE_GRAPH2");                  /* A2:1389-1409: one device call made the table, the prune and the graph */
	status("POST_PRE_GRAPH1");
	fprintf(stderr, "Pre Num nodes: %zu\npre nodes after pruning: %zu\n", vdjx_graph_pre_nodes(gg), n);
	status("POST_PRUNE_PRE_GRAPH1");
	status("POST_BUILD_GRAPH1");
	fprintf(stderr, "Num nodes: %zu\n", n);
	status("POST_BUILD_GRAPH2");
	vdjh_graph hg;
	memset(&hg, 0, sizeof hg);
	hg.n = n;
	hg.k = c.hp.k;
	char* kmers = (char*) malloc(n * (size_t) c.hp.k + 1);
	uint32_t* freq = (uint32_t*) malloc((n + 1) * 4);
	uint8_t *hv = (uint8_t*) malloc(n + 1), *hj = (uint8_t*) malloc(n + 1), *td = (uint8_t*) malloc(n + 1), *fd = (uint8_t*) malloc(n + 1);
	uint32_t *ti = (uint32_t*) malloc((n + 1) * 16), *fi = (uint32_t*) malloc((n + 1) * 16);
	VX(vdjx_graph_export(gg, NULL, NULL, freq, hv, hj, td, ti, fd, fi, kmers));
	hg.kmers = kmers; hg.freq = freq; hg.has_v = hv; hg.has_j = hj; hg.to_deg = td; hg.to_ids = ti; hg.from_deg = fd; hg.from_ids = fi;

	hook_ud ud;
	memset(&ud, 0, sizeof ud);
	ud.gx = gx; ud.mg = mg; ud.c = &c;
	ud.lin_num = c.lin_num; ud.dv_depth = c.div_depth;      /* (run state: their steps write them) */
	vdjh_hooks hk = {&ud, h_root_score, h_window_score, h_sam_body, vc, nv, jc, nj, h_status};
	vdjh_stats st;
	if (vdjh_assemble(&c.hp, &hg, &hk, "vdj_contigs.fa", "vdjer.dot", stdout, &st)) {
		fprintf(stderr, "%s\n", vdjh_last_error());
		return 1;
	}
	/* (no contig: the headers alone) */
	if (!ud.tables_ran && tables(&ud, NULL, NULL, 0, 0)) return 1;
	fprintf(stderr, "num root nodes: %zu\nProcessed roots: %zu\ncontig_candidates: %zu\nwindows scored: %zu valid: %zu\ncontigs: %zu\n",
	        st.n_roots, st.n_roots_accepted, st.n_contig_candidates, st.n_windows_scored, st.n_windows_valid, st.n_contigs_out);
	if (mg) {
		fprintf(stderr, "%llu bytes sent by rank 0 in all\n", (unsigned long long) vdjx_mgpu_bytes_sent(mg));
		if (vdjx_mgpu_finish(mg)) { fprintf(stderr, "%s\n", vdjx_mgpu_last_error()); return 1; }
	}
	for (int r = 1; r < c.gpus; r++) {                    /* the ranks have been released: they end, well */
		while (g_kid_state[r] == 0) {
			int st_ = 0;
			const pid_t p = waitpid(g_kids[r], &st_, 0);
			if (p == g_kids[r]) {
				g_kid_state[r] = (WIFEXITED(st_) && WEXITSTATUS(st_) == 0) ? 1 : 2;
				if (g_kid_state[r] == 2) fprintf(stderr, "rank %d ended with %s %d\n", r, WIFSIGNALED(st_) ? "signal" : "status", WIFSIGNALED(st_) ? WTERMSIG(st_) : WEXITSTATUS(st_));
			}
			else if (p < 0 && errno != EINTR) {
				/* reaped by the SIGCHLD handler -- which may be running on ANOTHER thread of this process (the GPU runtime has some,
				 * and a signal goes to any thread that does not block it): between its waitpid and its note of the outcome this
				 * thread can get here.  Its note comes within microseconds; a rank it found to have failed ends the process there. */
				for (int spin = 0; spin < 5000 && g_kid_state[r] == 0; spin++) usleep(1000);
				break;
			}
		}
		if (g_kid_state[r] != 1) { fprintf(stderr, "rank %d failed\n", r); return 1; }
	}
	status("FINIS");
	tables_summary(&ud);
	fflush(stdout);
	fflush(stderr);
	/* the outputs are written; the orderly teardown of a context that holds gigabytes (unmapping the workspaces piece by piece, the
	 * runtime's own exit handlers) took 160 ms of a 530 ms run at 400 k pairs -- the process ends instead and the driver reclaims what
	 * it held, as for any process.  VDJX_CLEAN_EXIT=1 keeps the teardown (leak checks). */
	if (!vdjx_env_set("VDJX_CLEAN_EXIT")) _exit(0);
	vdjx_graph_free(gg);
	if (mg) vdjx_mgpu_free(mg);
	vdjx_pool_free(px);
	vdjx_shutdown(gx);
	return 0;
}
