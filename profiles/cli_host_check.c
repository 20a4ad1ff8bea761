/* cli_host_check.c -- parse() of vdjer_amd/csrc/host/vdjer_cli.c on its own argv, stand-alone, for a run under a sanitizer (the option table
 * is offset arithmetic into cli).  From the repository's root, after the usual build:
 *   cc -std=gnu11 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include profiles/cli_host_check.c \
 *      vdjer_amd/csrc/host/vdjer_cli.c -Lvdjer_amd -lvdjhost -lvdjx -Wl,-rpath,$PWD/vdjer_amd -Wl,-rpath-link,/opt/rocm/lib -o cli_host_check
 *   python profiles/cli_host_check.py ./cli_host_check
 * Prints what parse() returned and a value of every kind, so that a value landing in the wrong field shows. */
#include <stdlib.h>

#include "../vdjer_amd/csrc/host/vdjer.h"

int main(int argc, char** argv) {
	cli c;
	const int rc = parse(argc, argv, &c);
	printf("parse %d", rc);
	if (!rc)
		printf(" in %s k %d mcs %.1f jc %c vf %s cr %s gpus %d quant %s boot %u seed %llu d %d total %s dist %d sym %d table %d link %d support %u depth %u div_boot %u "
		       "combine %d regs %zu weight %d class %d sub %u mut %u freq %d sample %s",
		       c.in, c.hp.k, c.hp.min_contig_score, c.hp.j_conserved, c.v_anchors, c.c_region, c.gpus, c.quant ? c.quant : "-", c.qb_b, (unsigned long long) c.qb_seed, c.d_calls,
		       c.total_count ? c.total_count : "-", c.lin_num, c.lin_sym, c.lin_table != NULL, c.lin_linkage, c.ts_b, c.div_depth, c.div_boot, c.sel_mean, c.nregs,
		       c.weight != NULL, c.tgt_cls, c.tgt_min_sub, c.tgt_min_mut, c.cons_num, c.sample);
	putchar('\n');
	for (size_t k = 0; k < c.nregs; k++) free(c.regs[k].name);      /* (what the options own lives as long as `vdjer` does) */
	free(c.regs); free(c.weight); free(c.lin_table);
	return rc ? 255 : 0;
}
