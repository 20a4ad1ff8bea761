/*
 * vdjer.h -- what the two files of the `vdjer` command line share: the options, which vdjer_cli.c reads and vdjer_main.c runs by.  Not
 * installed; the library's interface is include/vdjx.h.
 */
#ifndef VDJER_H
#define VDJER_H
#include <stdint.h>
#include <stdio.h>

#include "../../../include/vdjx.h"
#include "vdjh.h"

typedef struct vreg_line { char* name; int32_t iv[4]; } vreg_line;      /* a --v-regions line: the V record's name, cdr1 and cdr2 */

/* Every option's value, as the option table of vdjer_cli.c lays it down (the table names the flag of every field).  parse() fills it; from
 * then on it is read only.  A table's file is NULL when the table was not asked for. */
typedef struct {
	vdjh_params hp;
	const char* in;
	char v_anchors[4096], j_anchors[4096], source_sim_file[4096], vdj_fasta[4096];
	char v_region[64], c_region[64];       /* set_chain_info, params.c:8-35 (hg38 coordinates); --vr / --cr override */
	int anchor_mismatches, threads, gpus;
	const char* quant; uint32_t qb_b; uint64_t qb_seed;                /* qb_b 0: no bootstrap */
	const char* airr; int d_calls;
	const char *cfa, *isotypes, *clones, *total_count;
	const char* sample; char sample_buf[4096];                          /* --sample, or --in's base name up to its first '.' */
	const char* lineages; int lin_num, lin_den;                         /* --lineage-dist as lin_num / 10000 */
	const char* lin_model; int lin_sym; uint16_t* lin_table; vdjx_lineage_table_info lin_ti;      /* the model's distance table (NULL: Hamming) */
	const char* lin_threshold; int lin_linkage;
	const char *trees, *trees_nj, *trees_newick, *trees_mp, *trees_mp_newick; uint32_t ts_b; uint64_t ts_seed;      /* ts_b 0: no support column */
	const char* mutations;
	const char* diversity; uint32_t div_depth, div_boot; uint64_t div_seed;      /* div_depth 0: the total expected pairs */
	const char *selection, *v_regions, *targeting, *sel_test; int sel_mean, have_regs;
	vreg_line* regs; size_t nregs;                                      /* the lines of --v-regions */
	uint32_t* weight;                                                   /* the model of --targeting, [1024][4] (NULL: uniform) */
	const char *tgt_model, *tgt_counts; int tgt_cls; uint32_t tgt_min_sub, tgt_min_mut;
	const char* consensus; int cons_num;                                /* --consensus-min-freq as cons_num / 10000 */
} cli;

/* params.c:214-298 and validate_params, params.c:143-212: 0, or -1 after saying on stderr what is wrong; `--help` prints the usage and exits */
int parse(int argc, char** argv, cli* c);

#endif
