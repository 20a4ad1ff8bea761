/*
 * vdjer_cli.c -- the options of the `vdjer` command line (params.c:74-101, 214-298): ONE table of the flags (opts) and one of what a flag
 * needs beside it (needs).  parse() looks every flag up, reads the checked values, walks the requirements and then makes the few checks
 * that are no table rows; usage() prints the table.
 *
 * A new flag: a row in opts (its kind says how the text is read and checked, `off` where the value lands in cli, the last column is its
 * usage line), a row in needs if it is only meaningful beside another flag, a field in cli (vdjer.h) -- and the step of vdjer_main.c
 * that reads it.  A flag that fits no kind gets a handler (FN), not a kind of its own.
 */
#define _GNU_SOURCE
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "vdjer.h"

static int file_exists(const char* f) { struct stat b; return stat(f, &b) == 0; }

/* --lineage-dist: a decimal in [0, 1] with at most four digits after the point, read exactly (no strtod): at most one digit before the
 * point, at least one digit in all -> its numerator over 10000, or -1 (parse_lineage_dist of vdjer_amd/annot.py) */
static int lineage_dist_num(const char* s) {
	const char* dot = strchr(s, '.');
	const size_t wl = dot ? (size_t) (dot - s) : strlen(s), fl = dot ? strlen(dot + 1) : 0;
	if (wl + fl == 0 || wl > 1 || fl > 4 || strspn(s, "0123456789") != wl || (dot && strspn(dot + 1, "0123456789") != fl)) return -1;
	int v = wl ? (s[0] - '0') * 10000 : 0;
	for (size_t k = 0, scale = 1000; k < fl; k++, scale /= 10) v += (dot[1 + k] - '0') * (int) scale;
	return v <= 10000 ? v : -1;
}

/* the whole text as a decimal uint64: digits only, at least one, no overflow -> 0, or -1 */
static int whole_u64(const char* s, uint64_t* out) {
	uint64_t x = 0;
	if (!s[0]) return -1;
	for (; *s; s++) {
		if (*s < '0' || *s > '9') return -1;
		const uint64_t d = (uint64_t) (*s - '0');
		if (x > (UINT64_MAX - d) / 10) return -1;
		x = x * 10 + d;
	}
	*out = x;
	return 0;
}

/* --v-regions: lines `name cdr1_start cdr1_end cdr2_start cdr2_end`, separated by tabs or blanks; '#' lines and blank lines are skipped
 * (read_v_regions of vdjer_amd/annot.py).  The names meet the germline records later (sel_run). */
static int split_fields(char* line, char** f, int max) {
	int nf = 0;
	for (char* t = strtok(line, " \t\r\n"); t; t = strtok(NULL, " \t\r\n")) { if (nf < max) f[nf] = t; nf++; }
	return nf;
}

static int read_v_regions(const char* path, vreg_line** out, size_t* n_out) {
	FILE* fp = fopen(path, "r");
	if (!fp) { fprintf(stderr, "--v-regions: cannot read %s\n", path); return -1; }
	char* line = NULL;
	size_t lcap = 0, n = 0, cap = 0, no = 0;
	vreg_line* v = NULL;
	int rc = 0;
	while (!rc && getline(&line, &lcap, fp) >= 0) {
		no++;
		char* f[5];
		const int nf = split_fields(line, f, 5);
		if (!nf || f[0][0] == '#') continue;
		uint64_t x[4] = {0, 0, 0, 0};
		int bad = nf != 5;
		for (int k = 0; !bad && k < 4; k++) bad = whole_u64(f[1 + k], &x[k]) || x[k] > 2147483647u;
		if (bad) { fprintf(stderr, "--v-regions: %s line %zu: expected `name cdr1_start cdr1_end cdr2_start cdr2_end` with whole numbers\n", path, no); rc = -1; break; }
		for (int k = 0; k < 4; k += 2)
			if (x[k] > x[k + 1] || (x[k] == 0 && x[k + 1] != 0)) {
				fprintf(stderr, "--v-regions: %s line %zu: the interval %llu .. %llu (1 <= start <= end, or 0 0)\n", path, no, (unsigned long long) x[k], (unsigned long long) x[k + 1]);
				rc = -1;
			}
		for (size_t q = 0; !rc && q < n; q++)
			if (!strcmp(v[q].name, f[0])) { fprintf(stderr, "--v-regions: %s line %zu: the name %s is given twice\n", path, no, f[0]); rc = -1; }
		if (rc) break;
		if (n + 1 > cap) { cap = cap ? 2 * cap : 256; v = (vreg_line*) realloc(v, cap * sizeof *v); }
		v[n].name = strdup(f[0]);
		for (int k = 0; k < 4; k++) v[n].iv[k] = (int32_t) x[k];
		n++;
	}
	free(line);
	fclose(fp);
	*out = v;
	*n_out = n;
	return rc;
}

/* --targeting: exactly 1,024 lines `<5-mer> <wA> <wC> <wG> <wT>`, each 5-mer over ACGT once, whole decimal numbers below 2^32; '#' lines and
 * blank lines are skipped (read_targeting of vdjer_amd/annot.py) -> uint32 [1024][4] */
static int read_targeting(const char* flag, const char* path, uint32_t** out) {
	FILE* fp = fopen(path, "r");
	if (!fp) { fprintf(stderr, "%s: cannot read %s\n", flag, path); return -1; }
	uint32_t* w = (uint32_t*) calloc(4096, sizeof(uint32_t));
	unsigned char* seen = (unsigned char*) calloc(1024, 1);
	char* line = NULL;
	size_t lcap = 0, no = 0, got = 0;
	int rc = 0;
	while (getline(&line, &lcap, fp) >= 0) {
		no++;
		char* f[5];
		const int nf = split_fields(line, f, 5);
		if (!nf || f[0][0] == '#') continue;
		uint64_t x[4] = {0, 0, 0, 0};
		int bad = nf != 5 || strlen(f[0]) != 5 || strspn(f[0], "ACGT") != 5;
		for (int k = 0; !bad && k < 4; k++) bad = whole_u64(f[1 + k], &x[k]) || x[k] > 4294967295ull;
		if (bad) { fprintf(stderr, "%s: %s line %zu: expected `<5-mer over ACGT> <wA> <wC> <wG> <wT>` with whole numbers below 2^32\n", flag, path, no); rc = -1; break; }
		int idx = 0;
		for (int k = 0; k < 5; k++) idx = 4 * idx + (int) (strchr("ACGT", f[0][k]) - "ACGT");
		if (seen[idx]) { fprintf(stderr, "%s: %s line %zu: the 5-mer %s is given twice\n", flag, path, no, f[0]); rc = -1; break; }
		seen[idx] = 1;
		got++;
		for (int k = 0; k < 4; k++) w[4 * idx + k] = (uint32_t) x[k];
	}
	if (!rc && got != 1024) { fprintf(stderr, "%s: %s holds %zu 5-mers, expected every one of the 1024 once\n", flag, path, got); rc = -1; }
	free(line);
	free(seen);
	fclose(fp);
	if (rc) { free(w); w = NULL; }
	*out = w;
	return rc;
}

/* ---- the option table --------------------------------------------------------------------------------------------------------------- */
enum {
	TEXT, PATH, INT, FLOAT, CHAR, NOVAL, FN,      /* taken as they come, in the order of the command line: a later flag overrides an earlier one */
	RANGE, SEED, FRAC, WORD, DIGITS               /* checked, once the whole command line is read: the last value of a flag counts */
};

typedef struct {
	const char* name;
	int kind;
	size_t off;                       /* where the value lands in cli */
	uint64_t lo, hi, def;             /* RANGE: lo .. hi and the default; SEED, FRAC: the default; PATH: hi is the buffer's size */
	const char *words, *say;          /* WORD: "a|b|c" -> 0, 1, 2 (default 0), and how a refusal names them */
	int (*fn)(cli*, const char*);     /* FN: 0, or not 0 after saying what is wrong: the parse ends there */
	const char* usage;                /* its line of the usage text (NULL: accepted, not listed) */
} opt;

/* --chain: the presets of set_chain_info, params.c:8-35, and the loci's hg38 coordinates */
static int set_chain(cli* c, const char* v) {
	if (vdjh_set_chain(&c->hp, v)) { fprintf(stderr, "%s\n", vdjh_last_error()); return -1; }
	const char* vr = !strcmp(v, "IGH") ? "chr14:105566277-106879844" : !strcmp(v, "IGL") ? "chr22:22026076-22922913" : "chr2:89851758-90235368";
	const char* cr = !strcmp(v, "IGH") ? "chr14:105566277-105939754" : !strcmp(v, "IGL") ? "chr22:22895375-22922913" : "chr2:88857361-88857683";
	snprintf(c->v_region, sizeof c->v_region, "%s", vr);
	snprintf(c->c_region, sizeof c->c_region, "%s", cr);
	return 0;
}

static int set_ref_dir(cli* c, const char* v) {
	snprintf(c->v_anchors, sizeof c->v_anchors, "%s/v_index", v);
	snprintf(c->j_anchors, sizeof c->j_anchors, "%s/j_index", v);
	snprintf(c->source_sim_file, sizeof c->source_sim_file, "%s/v_region.fa", v);
	snprintf(c->vdj_fasta, sizeof c->vdj_fasta, "%s/ig_vdj.fa", v);
	return 0;
}

#define AT(field) offsetof(cli, field)
#define O_TEXT(n, f, u)  {.name = n, .kind = TEXT, .off = AT(f), .usage = u}
#define O_PATH(n, f, u)  {.name = n, .kind = PATH, .off = AT(f), .hi = sizeof ((cli*) 0)->f, .usage = u}
#define O_INT(n, f, u)   {.name = n, .kind = INT, .off = AT(f), .usage = u}
#define O_FN(n, h, u)    {.name = n, .kind = FN, .fn = h, .usage = u}
#define O_RANGE(n, f, a, b, d, u) {.name = n, .kind = RANGE, .off = AT(f), .lo = a, .hi = b, .def = d, .usage = u}
#define O_SEED(n, f, u)  {.name = n, .kind = SEED, .off = AT(f), .def = 1, .usage = u}
#define O_FRAC(n, f, d, u) {.name = n, .kind = FRAC, .off = AT(f), .def = d, .usage = u}
#define O_WORD(n, f, w, s, u) {.name = n, .kind = WORD, .off = AT(f), .words = w, .say = s, .usage = u}

/* in the order of the usage text; the checked values are read, and refused, in this order too */
static const opt opts[] = {
	O_TEXT("--in", in, "--in <input BAM (with .bai), or the extracted reads as text (see vdjer_main.c)>"),
	O_FN("--chain", set_chain, "--chain <IGH|IGK|IGL>"),
	O_FN("--ref-dir", set_ref_dir, "--ref-dir </path/to/vdjer/ref/dir>"),
	O_INT("--mf", hp.min_node_freq, "--mf <min node frequency (default: 3)>"),
	O_INT("--mq", hp.min_base_quality, "--mq <min base quality (default: 90)>"),
	{.name = "--mcs", .kind = FLOAT, .off = AT(hp.min_contig_score), .usage = "--mcs <min contig score (default: -5)"},
	O_INT("--t", threads, "--t <threads (default: 1)"),
	O_INT("--am", anchor_mismatches, "--am <anchor mismatches (default: 4)"),
	O_INT("--miw", hp.vj_min_win, "--miw/--maw <min/max window between conserved amino acids>"),
	O_INT("--maw", hp.vj_max_win, NULL),
	{.name = "--jc", .kind = CHAR, .off = AT(hp.j_conserved), .usage = "--jc <conserved J amino acid (W|F)"},
	O_INT("--ws", hp.window_span, "--ws <window span (default: 486)"),
	O_INT("-jext", hp.j_extension, "--jext <J extension (default: 162)"),      /* sic: params.c:262 reads one dash, params.c:88 prints two */
	O_INT("--ins", hp.insert_len, "--ins <expected / median insert length>"),
	O_INT("--rf", hp.read_filter_floor, "--rf <read filter floor (default: 1)"),
	O_INT("--k", hp.k, "--k <kmer size (default: 35)>"),
	O_INT("--vk", hp.vregion_kmer_size, "--vk <vregion kmer size (default: 15)>"),
	O_INT("--mrs", hp.min_source_homology_score, "--mrs <min source node homology score (default: 30)"),
	O_INT("--rs", hp.filter_read_span, "--rs <read span distance (default: 35)>"),
	O_INT("--ms", hp.filter_mate_span, "--ms <mate span distance (default: 48)>"),
	O_INT("--e0", hp.eval_start, "--e0/--e1 <start/stop position for contig filtering (default: 52/411)>"),
	O_INT("--e1", hp.eval_stop, NULL),
	O_INT("--wo", hp.window_overlap_check_size, "--wo <window overlap check size>"),
	O_PATH("--vf", v_anchors, NULL),
	O_PATH("--jf", j_anchors, NULL),
	O_PATH("--vdjf", vdj_fasta, NULL),
	O_PATH("--vr", v_region, NULL),
	O_PATH("--cr", c_region, NULL),
	O_PATH("--rms", source_sim_file, NULL),
	/* not in the reference from here on */
	O_INT("--gpus", gpus, "--gpus <GPUs of this node to shard the k-mer table over (default: 1)>"),
	O_TEXT("--quant", quant, "--quant <file: expected read pairs per contig, an RSEM isoforms.results table (one GPU only)>"),
	O_RANGE("--quant-boot", qb_b, 1, 1024, 0, "--quant-boot <B: with --quant, bootstrap the placed pairs B times (a whole number in 1 .. 1024): boot_mean, boot_sd, boot_lower, boot_upper>"),
	O_SEED("--quant-seed", qb_seed, "--quant-seed <seed of the --quant-boot draws, a whole number below 2^64 (default: 1)>"),
	O_TEXT("--airr", airr, "--airr <file: V/J calls of every contig against ig_vdj.fa, an AIRR Rearrangement table>"),
	{.name = "--d-calls", .kind = NOVAL, .off = AT(d_calls), .usage = "--d-calls (no value; with --airr: the D gene between the V and the J hit against the D records of ig_vdj.fa, and np1 / np2)"},
	O_TEXT("--cfa", cfa, "--cfa <constant-region FASTA for --isotypes / --clones>"),
	O_TEXT("--isotypes", isotypes, "--isotypes <file: isotype call of every contig's last 48 bases against --cfa>"),
	O_TEXT("--clones", clones, "--clones <file: the clustered clone table of this sample (one GPU only)>"),
	O_TEXT("--sample", sample, "--sample <name in the clone table (default: the input's base name up to its first '.')>"),
	{.name = "--total-count", .kind = DIGITS, .off = AT(total_count), .usage = "--total-count <whole number for the clone table's total_count column (default: N/A)>"},
	O_TEXT("--lineages", lineages, "--lineages <file: clonal lineages of the contigs, single linkage on the junctions inside a V gene / J gene / length bucket>"),
	O_FRAC("--lineage-dist", lin_num, 1500, "--lineage-dist <largest linked distance as a fraction of the junction length, in [0,1], at most 4 decimals (default: 0.15)>"),
	O_TEXT("--lineage-model", lin_model, "--lineage-model <file: with --lineages, a 5-mer targeting model as --targeting reads it: link under its substitution distance, --lineage-dist in mean mismatches>"),
	O_WORD("--lineage-symmetry", lin_sym, "avg|min", "avg (both directions added) or min (twice the cheaper)",
	       "--lineage-symmetry <avg|min: with --lineage-model, add both directions of a mismatch (default: avg) or take twice the cheaper>"),
	O_TEXT("--lineage-threshold", lin_threshold, "--lineage-threshold <file: with --lineages, choose the threshold from the distances to the nearest neighbour (the valley between their two modes; --lineage-dist stands when there is none) and write their histogram and smoothed density>"),
	O_WORD("--lineage-link", lin_linkage, "single|complete|average", "single, complete or average",
	       "--lineage-link <single|complete|average: with --lineages, the linkage the lineages are cut at the threshold under (default: single; where distances tie, complete and average depend on the contigs' order)>"),
	O_TEXT("--trees", trees, "--trees <file: with --lineages, the minimum spanning tree inside every lineage: parent, distance and depth of every contig>"),
	O_TEXT("--trees-nj", trees_nj, "--trees-nj <file: with --lineages, the neighbour-joining tree inside every lineage with its inferred ancestors: a row per node>"),
	O_TEXT("--trees-newick", trees_newick, "--trees-newick <file: with --trees-nj, one Newick line per lineage of two and more members>"),
	O_TEXT("--trees-mp", trees_mp, "--trees-mp <file: with --lineages, the neighbour-joining tree of every lineage after a search over nearest-neighbour interchanges for fewer mutations: a row per node>"),
	O_TEXT("--trees-mp-newick", trees_mp_newick, "--trees-mp-newick <file: with --trees-mp, one Newick line per lineage of two and more members, lengths in mutations>"),
	O_RANGE("--tree-support", ts_b, 1, 1024, 0, "--tree-support <B: with --trees, a support column from B delete-half jackknife replicates, a whole number in 1 .. 1024>"),
	O_SEED("--tree-seed", ts_seed, "--tree-seed <seed of the replicates' columns, a whole number below 2^64 (default: 1)>"),
	O_TEXT("--mutations", mutations, "--mutations <file: every contig beside its V(D)J germline, and the V segment's replacement / silent / stop mutation counts>"),
	O_TEXT("--diversity", diversity, "--diversity <file: with --lineages and --quant or --clones, the Hill diversity curve of the lineages, orders 0.0 .. 4.0, bootstrapped>"),
	O_RANGE("--diversity-depth", div_depth, 1, 2147483647, 0, "--diversity-depth <n: draws per bootstrap replicate, a whole number in 1 .. 2147483647 (default: the lineages' total expected pairs)>"),
	O_RANGE("--diversity-boot", div_boot, 1, 4096, 200, "--diversity-boot <B: bootstrap replicates, a whole number in 1 .. 4096 (default: 200)>"),
	O_SEED("--diversity-seed", div_seed, "--diversity-seed <seed of the draws, a whole number below 2^64 (default: 1)>"),
	O_TEXT("--selection", selection, "--selection <file: selection strength (BASELINe) of the V mutations: observed and expected R / S and the posterior of sigma per contig, lineage (with --lineages) and sample>"),
	O_TEXT("--v-regions", v_regions, "--v-regions <file: with --selection, lines `name cdr1_start cdr1_end cdr2_start cdr2_end` (1-based, inclusive, 0 0: none) of the V records: rows fwr and cdr>"),
	O_WORD("--selection-combine", sel_mean, "shared|mean", "shared or mean",
	       "--selection-combine <shared|mean: with --selection, the lineage and sample rows as one shared sigma (default) or as BASELINe's mean of the members' sigmas (their densities convolved)>"),
	O_TEXT("--selection-test", sel_test, "--selection-test <file: with --selection and --v-regions, cdr against fwr per lineage and sample: P(sigma_cdr > sigma_fwr), two-sided p-value, Benjamini-Hochberg fdr>"),
	O_TEXT("--targeting", targeting, "--targeting <file: with --selection, 1024 lines `<5-mer> <wA> <wC> <wG> <wT>`, whole numbers below 2^32 (default: uniform)>"),
	O_TEXT("--targeting-model", tgt_model, "--targeting-model <file: the sample's own 5-mer targeting model, in the format --targeting reads, learnt from the V mutations (a lineage of --lineages counted once)>"),
	O_WORD("--targeting-class", tgt_cls, "s|rs", "s (silent changes only) or rs (silent and replacement)",
	       "--targeting-class <s|rs: with --targeting-model, learn from silent changes only (default: s) or from silent and replacement>"),
	O_RANGE("--targeting-min-sub", tgt_min_sub, 1, 4294967295u, 50, "--targeting-min-sub <n: with --targeting-model, changes a 5-mer needs for its own substitution row, a whole number in 1 .. 4294967295 (default: 50)>"),
	O_RANGE("--targeting-min-mut", tgt_min_mut, 1, 4294967295u, 500, "--targeting-min-mut <n: with --targeting-model, changes a 5-mer needs for its own mutability, a whole number in 1 .. 4294967295 (default: 500)>"),
	O_TEXT("--targeting-counts", tgt_counts, "--targeting-counts <file: with --targeting-model, the observed and opportunity counts per 5-mer and the levels used>"),
	O_TEXT("--consensus", consensus, "--consensus <file: with --lineages, the consensus V sequence of every lineage (and of every contig in none) beside its germline, and its mutation counts>"),
	O_FRAC("--consensus-min-freq", cons_num, 6000, "--consensus-min-freq <share of a column's votes its winner needs, in [0,1], at most 4 decimals (default: 0.6; 0: the most common)>"),
};
#define N_OPTS (sizeof opts / sizeof opts[0])

/* `flag` is refused unless `need` (or `or_need`) is given too: "<flag> <what>: it needs <need> <arg>" */
static const struct { const char *flag, *what, *need, *or_need, *arg; } needs[] = {
	{"--quant-boot", "bootstraps the --quant table", "--quant", NULL, "<file>"},
	{"--quant-seed", "is the seed of the --quant-boot replicates", "--quant-boot", NULL, "<B>"},
	{"--d-calls", "adds the D call to the --airr table", "--airr", NULL, "<file>"},
	{"--lineage-dist", "is the threshold of the --lineages table", "--lineages", NULL, "<file>"},
	{"--lineage-model", "is the distance model of the --lineages table", "--lineages", NULL, "<file>"},
	{"--lineage-symmetry", "is the symmetry of the --lineage-model distance", "--lineage-model", NULL, "<file>"},
	{"--lineage-threshold", "chooses the threshold of the --lineages table", "--lineages", NULL, "<file>"},
	{"--lineage-link", "is the linkage of the --lineages table", "--lineages", NULL, "<file>"},
	{"--trees", "writes the tree inside every lineage of the --lineages table", "--lineages", NULL, "<file>"},
	{"--trees-nj", "writes the neighbour-joining tree inside every lineage of the --lineages table", "--lineages", NULL, "<file>"},
	{"--trees-newick", "writes the trees of --trees-nj as Newick lines", "--trees-nj", NULL, "<file>"},
	{"--trees-mp", "writes the maximum-parsimony tree inside every lineage of the --lineages table", "--lineages", NULL, "<file>"},
	{"--trees-mp-newick", "writes the trees of --trees-mp as Newick lines", "--trees-mp", NULL, "<file>"},
	{"--tree-support", "adds the support column to the --trees table", "--trees", NULL, "<file>"},
	{"--tree-seed", "is the seed of the --tree-support replicates", "--tree-support", NULL, "<B>"},
	{"--diversity", "is the diversity of the lineages of the --lineages table", "--lineages", NULL, "<file>"},
	{"--diversity", "weighs the lineages by the quant step's expected counts", "--quant", "--clones", "<file>"},
	{"--diversity-depth", "is the draws of a --diversity replicate", "--diversity", NULL, "<file>"},
	{"--diversity-boot", "is the number of --diversity replicates", "--diversity", NULL, "<file>"},
	{"--diversity-seed", "is the seed of the --diversity replicates", "--diversity", NULL, "<file>"},
	{"--v-regions", "is the region map of the --selection table", "--selection", NULL, "<file>"},
	{"--targeting", "is the targeting model of the --selection table", "--selection", NULL, "<file>"},
	{"--selection-combine", "is how the --selection table combines the members of a row", "--selection", NULL, "<file>"},
	{"--selection-test", "compares the densities of the --selection table", "--selection", NULL, "<file>"},
	{"--selection-test", "compares the cdr rows with the fwr rows", "--v-regions", NULL, "<file>"},
	{"--consensus", "is the consensus of every lineage of the --lineages table", "--lineages", NULL, "<file>"},
	{"--consensus-min-freq", "is the threshold of the --consensus table", "--consensus", NULL, "<file>"},
	{"--targeting-class", "is the mutation class of the --targeting-model file", "--targeting-model", NULL, "<file>"},
	{"--targeting-min-sub", "is a threshold of the --targeting-model file", "--targeting-model", NULL, "<file>"},
	{"--targeting-min-mut", "is a threshold of the --targeting-model file", "--targeting-model", NULL, "<file>"},
	{"--targeting-counts", "is the counts behind the --targeting-model file", "--targeting-model", NULL, "<file>"},
};

static void usage(void) {
	fprintf(stderr, "vdjer \n");
	for (size_t k = 0; k < N_OPTS; k++)
		if (opts[k].usage) fprintf(stderr, "\t%s\n", opts[k].usage);
}

/* the flag's row in opts, or N_OPTS */
static size_t find_opt(const char* name) {
	size_t k = 0;
	while (k < N_OPTS && strcmp(opts[k].name, name)) k++;
	return k;
}

/* a value of the unchecked kinds */
static int take(cli* c, const opt* o, const char* v) {
	void* at = (char*) c + o->off;
	switch (o->kind) {
	case TEXT: *(const char**) at = v; break;
	case PATH: snprintf((char*) at, (size_t) o->hi, "%s", v); break;
	case INT: *(int*) at = atoi(v); break;
	case FLOAT: *(float*) at = (float) atof(v); break;
	case CHAR: *(int*) at = v[0]; break;
	case FN: return o->fn(c, v);
	}
	return 0;
}

/* a value of the checked kinds (v NULL: the default) -> 0, or -1 after the refusal */
static int take_checked(cli* c, const opt* o, const char* v) {
	void* at = (char*) c + o->off;
	uint64_t x = o->def;
	int n = (int) o->def;
	switch (o->kind) {
	case RANGE:
		if (v && (whole_u64(v, &x) || x < o->lo || x > o->hi)) {
			fprintf(stderr, "%s must be a whole decimal number in %llu .. %llu: %s\n", o->name, (unsigned long long) o->lo, (unsigned long long) o->hi, v);
			return -1;
		}
		*(uint32_t*) at = (uint32_t) x;
		break;
	case SEED:
		if (v && whole_u64(v, &x)) { fprintf(stderr, "%s must be a whole decimal number below 2^64: %s\n", o->name, v); return -1; }
		*(uint64_t*) at = x;
		break;
	case FRAC:
		if (v && (n = lineage_dist_num(v)) < 0) { fprintf(stderr, "%s must be a decimal in [0, 1] with at most four digits after the point: %s\n", o->name, v); return -1; }
		*(int*) at = n;
		break;
	case WORD:
		n = 0;
		for (const char* w = o->words; v; n++) {      /* the place of v among the words */
			const size_t wl = strcspn(w, "|");
			if (wl == strlen(v) && !memcmp(w, v, wl)) break;
			if (!w[wl]) { fprintf(stderr, "%s must be %s: %s\n", o->name, o->say, v); return -1; }
			w += wl + 1;
		}
		*(int*) at = n;
		break;
	case DIGITS:
		if (v && (!v[0] || strspn(v, "0123456789") != strlen(v))) { fprintf(stderr, "%s must be a whole decimal number: %s\n", o->name, v); return -1; }
		*(const char**) at = v;
		break;
	}
	return 0;
}

int parse(int argc, char** argv, cli* c) {
	const char* given[N_OPTS] = {NULL};      /* per row of opts: the flag's last value (the flag itself where it has none), NULL: not given */
	memset(c, 0, sizeof *c);
	vdjh_default_params(&c->hp);
	c->anchor_mismatches = 4;
	c->threads = 1;
	c->gpus = 1;
	c->lin_den = 10000;
	/* the lookup: positional "--flag value" pairs from argv[1]; unknown flags only warn */
	for (int i = 1; i < argc; i += 2) {
		const char* a = argv[i];
		if (!strcmp(a, "--help")) { usage(); exit(0); }
		const size_t k = find_opt(a);
		if (k < N_OPTS && opts[k].kind == NOVAL) { *(int*) ((char*) c + opts[k].off) = 1; given[k] = a; i--; continue; }
		if (i + 1 >= argc) { fprintf(stderr, "Missing value for param: %s\n", a); usage(); return -1; }
		if (k == N_OPTS) { fprintf(stderr, "Invalid param: %s\n", a); continue; }
		given[k] = argv[i + 1];
		if (opts[k].kind < RANGE && take(c, &opts[k], given[k])) return -1;
	}
	int ok = 1;
	/* the values */
	for (size_t k = 0; k < N_OPTS; k++)
		if (opts[k].kind >= RANGE && take_checked(c, &opts[k], given[k])) ok = 0;
	/* the requirements */
	for (size_t r = 0; r < sizeof needs / sizeof needs[0]; r++) {
		if (!given[find_opt(needs[r].flag)] || given[find_opt(needs[r].need)] || (needs[r].or_need && given[find_opt(needs[r].or_need)])) continue;
		fprintf(stderr, "%s %s: it needs %s %s", needs[r].flag, needs[r].what, needs[r].need, needs[r].arg);
		if (needs[r].or_need) fprintf(stderr, " or %s %s", needs[r].or_need, needs[r].arg);
		fputc('\n', stderr);
		ok = 0;
	}
	/* what is no row of a table: validate_params, params.c:143-212 */
	if (!c->in) { fprintf(stderr, "Input must be specified\n"); ok = 0; }
	else if (!file_exists(c->in)) { fprintf(stderr, "Could not find input file: %s\n", c->in); ok = 0; }
	if (!c->v_anchors[0]) { fprintf(stderr, "V anchor file must be specified\n"); ok = 0; }
	else if (!file_exists(c->v_anchors)) { fprintf(stderr, "Could not locate v_index file: %s\n", c->v_anchors); ok = 0; }
	if (!c->j_anchors[0]) { fprintf(stderr, "J anchor file must be specified\n"); ok = 0; }
	else if (!file_exists(c->j_anchors)) { fprintf(stderr, "Could not locate j_index file: %s\n", c->j_anchors); ok = 0; }
	if (!c->source_sim_file[0]) { fprintf(stderr, "source_sim_file file must be specified\n"); ok = 0; }
	if (c->hp.j_conserved != 'W' && c->hp.j_conserved != 'F') { fprintf(stderr, "Conserved J AA must be W or F: %c\n", c->hp.j_conserved); ok = 0; }
	if (c->hp.insert_len <= 0) { fprintf(stderr, "insert_len must be specified and > 0\n"); ok = 0; }
	/* (vdjx_vregion_load's limit, said here: before the input is read, let alone a pool loaded) */
	if (c->hp.vregion_kmer_size < 2 || c->hp.vregion_kmer_size > 16) { fprintf(stderr, "--vk: vregion k-mer size %d outside [2,16]\n", c->hp.vregion_kmer_size); ok = 0; }
	if (c->isotypes && !c->cfa) { fprintf(stderr, "--isotypes needs the constant-region sequences: --cfa <fasta>\n"); ok = 0; }
	if (c->cfa) {
		FILE* fp = fopen(c->cfa, "r");
		if (!fp) { fprintf(stderr, "--cfa: cannot read the constant-region FASTA %s\n", c->cfa); ok = 0; }
		else fclose(fp);
	}
	/* the files a step reads are read here, before any GPU work; each only beside the table it belongs to.  --lineage-model must exist
	 * beforehand: a run does not read the --targeting-model file it is writing itself, and neither does its --selection table */
	if (c->lin_model && c->lineages) {
		uint32_t* w = NULL;
		if (read_targeting("--lineage-model", c->lin_model, &w)) ok = 0;
		else {
			c->lin_table = (uint16_t*) calloc(4096, sizeof(uint16_t));
			if (vdjx_lineage_distance_table(w, c->lin_table, &c->lin_ti)) { fprintf(stderr, "--lineage-model: %s\n", vdjx_last_error()); ok = 0; }
			free(w);
		}
	}
	if (c->v_regions && c->selection && read_v_regions(c->v_regions, &c->regs, &c->nregs)) ok = 0;
	if (c->targeting && c->selection && read_targeting("--targeting", c->targeting, &c->weight)) ok = 0;
	c->have_regs = c->v_regions != NULL;
	if (!c->sample && c->in) {                /* the input's base name up to its first '.' */
		const char* b = strrchr(c->in, '/');
		snprintf(c->sample_buf, sizeof c->sample_buf, "%s", b ? b + 1 : c->in);
		c->sample_buf[strcspn(c->sample_buf, ".")] = 0;
		c->sample = c->sample_buf;
	}
	if (!ok) { usage(); return -1; }
	if (c->hp.min_base_quality >= 255) c->hp.min_base_quality = 254;      /* A2:1514-1516 */
	return 0;
}
