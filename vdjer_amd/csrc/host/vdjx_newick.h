/* vdjx_newick.h -- the Newick writer of `vdjer --trees-newick` (plain C, no GPU; profiles/nj_host_check.cpp runs it under a sanitizer).
 * A tree is given as vdjx_tree_nj returns it: parent[] over the slots.  newick_children lists every slot's children in ascending slot
 * (a counting sort: O(nodes)); newick_write prints the tree below one root as (<children>)'<label>':<length / 65536 as %.4f>, the root
 * itself without a length, then ";".  No recursion: a lineage may be thousands of nodes deep.  The same bytes as
 * vdjer_amd/annot.py's tree_nj_newick. */
#ifndef VDJX_NEWICK_H
#define VDJX_NEWICK_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

/* kid_off[nodes + 1], kid[nodes]: the children of slot s are kid[kid_off[s] .. kid_off[s + 1]), ascending.  -1: a parent outside
 * -1 .. nodes - 1, or itself */
static inline int newick_children(const int32_t* parent, size_t nodes, size_t* kid_off, uint32_t* kid) {
	for (size_t s = 0; s <= nodes; s++) kid_off[s] = 0;
	for (size_t s = 0; s < nodes; s++) {
		if (parent[s] < -1 || (parent[s] >= 0 && ((size_t) parent[s] >= nodes || (size_t) parent[s] == s))) return -1;
		if (parent[s] >= 0) kid_off[parent[s] + 1]++;
	}
	for (size_t s = 0; s < nodes; s++) kid_off[s + 1] += kid_off[s];
	size_t* fill = (size_t*) malloc((nodes + 1) * sizeof(size_t));
	if (!fill) return -1;
	for (size_t s = 0; s < nodes; s++) fill[s] = kid_off[s];
	for (size_t s = 0; s < nodes; s++)
		if (parent[s] >= 0) kid[fill[parent[s]]++] = (uint32_t) s;
	free(fill);
	return 0;
}

typedef void (*newick_label_fn)(FILE* fp, size_t slot, void* ud);

/* -1: out of memory, or more than `nodes` steps down (a cycle in parent[]: never from vdjx_tree_nj) */
static inline int newick_write(FILE* fp, size_t root, const int64_t* length, size_t nodes, const size_t* kid_off, const uint32_t* kid,
                               newick_label_fn label, void* ud) {
	size_t* node = (size_t*) malloc((nodes + 1) * sizeof(size_t));
	size_t* at = (size_t*) malloc((nodes + 1) * sizeof(size_t));
	if (!node || !at || root >= nodes) { free(node); free(at); return -1; }
	size_t top = 0;
	int rc = 0;
	node[0] = root;
	at[0] = kid_off[root];
	if (kid_off[root + 1] > kid_off[root]) fputc('(', fp);
	for (;;) {
		const size_t s = node[top];
		if (at[top] < kid_off[s + 1]) {
			if (at[top] > kid_off[s]) fputc(',', fp);
			const size_t c = kid[at[top]++];
			if (top + 1 >= nodes) { rc = -1; break; }
			node[++top] = c;
			at[top] = kid_off[c];
			if (kid_off[c + 1] > kid_off[c]) fputc('(', fp);
			continue;
		}
		if (kid_off[s + 1] > kid_off[s]) fputc(')', fp);
		fputc('\'', fp);
		label(fp, s, ud);
		fputc('\'', fp);
		if (top == 0) break;
		fprintf(fp, ":%.4f", (double) length[s] / 65536.0);
		top--;
	}
	fputc(';', fp);
	free(node);
	free(at);
	return rc;
}

#endif
