"""Germline records for contig annotation (vdjx_germline_load, include/vdjx.h): the FASTA reader and the name / class rules that
`vdjer --airr` applies in C (vdjer_main.c) as well; and the three rules `vdjer --isotypes` / `--clones` apply to the called names (the
reference's post_process/call_isotypes.py and collect_vdjer_stats.py)."""
from __future__ import annotations


def read_fasta(path: str):
    """[(header without '>', sequence)] of a FASTA file (sequence lines joined)"""
    out, head, seq = [], None, []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                if head is not None:
                    out.append((head, "".join(seq)))
                head, seq = line[1:], []
            elif head is not None:
                seq.append(line)
    if head is not None:
        out.append((head, "".join(seq)))
    return out


def parse_name(header: str) -> str:
    """the header's first token, or its second '|' field when the token has one (IMGT/GENE-DB headers)"""
    tok = header.split()[0] if header.split() else ""
    if "|" in tok:
        return tok.split("|")[1]
    return tok


def parse_class(name: str) -> str:
    """the 4th character of IG[HKL]* / TR[ABDG]* names, the 1st otherwise ('' for an empty name)"""
    if len(name) >= 4 and ((name[:2] == "IG" and name[2] in "HKL") or (name[:2] == "TR" and name[2] in "ABDG")):
        return name[3]
    return name[:1]


def clean_seq(seq: str) -> str:
    """upper case; IMGT gaps ('.') and whitespace dropped"""
    return "".join(ch for ch in seq.upper() if ch != "." and not ch.isspace())


def parse_record(header: str, seq: str):
    """(name, class, sequence) of a FASTA record"""
    name = parse_name(header)
    return name, parse_class(name), clean_seq(seq)


DCALL_WINDOW = 256                                          # VDJX_DCALL_WINDOW (include/vdjx.h)


def d_window(v, j):
    """the window `vdjer --airr --d-calls` hands to vdjx_dcall, from the V and the J hits ({field: array} as Context.annotate returns
    them) -> (start, length) int32 arrays: with a V and a J hit (gene >= 0 and score > 0) the bases strictly between them (0-based start
    v.seq_end, length j.seq_start - 1 - v.seq_end); length 0 (and start 0) when the hits abut or overlap, when more than 256 bases lie
    between them, or without a V hit or a J hit"""
    import numpy as np
    has = (np.asarray(v["gene"]) >= 0) & (np.asarray(v["score"]) > 0) & (np.asarray(j["gene"]) >= 0) & (np.asarray(j["score"]) > 0)
    start = np.asarray(v["seq_end"]).astype(np.int64)
    length = np.asarray(j["seq_start"]).astype(np.int64) - 1 - start
    ok = has & (length > 0) & (length <= DCALL_WINDOW)
    return np.where(ok, start, 0).astype(np.int32), np.where(ok, length, 0).astype(np.int32)


def gene_of(name: str) -> str:
    """the gene of an allele name: the text before the first '*' (IGHG1*01 -> IGHG1)"""
    return name.split("*", 1)[0]


def _distinct(items) -> str:
    out = []
    for x in items:
        if x not in out:
            out.append(x)
    return ",".join(out)


def subtypes(names) -> str:
    """the isotype of a call: the distinct first four characters of the genes (IGHG1 -> IGHG), in order of first appearance"""
    return _distinct(gene_of(x)[:4] for x in names)


def vq_gene(names) -> str:
    """get_vq_gene's normalisation (collect_vdjer_stats.py): per name the text before '*', every 'D' deleted (IGHV1-69D -> IGHV1-69,
    IGKV1D-39 -> IGKV1-39), then what lies before a second '-' (IGHV3-30-5 -> IGHV3-30); the distinct results in order of first
    appearance"""
    return _distinct("-".join(gene_of(x).replace("D", "").split("-")[:2]) for x in names)


LINEAGE_NONE = 0xFFFFFFFF                                   # VDJX_LINEAGE_NONE (include/vdjx.h)
LINEAGE_MAXLEN = 255                                        # VDJX_LINEAGE_MAXLEN
LINEAGE_LINKAGE = {"single": 0, "complete": 1, "average": 2}    # --lineage-link <name> -> vdjx_lineage_link_params.linkage
LINEAGE_LINK_NAMES = tuple(LINEAGE_LINKAGE)                 # ... and back: LINEAGE_LINK_NAMES[linkage]
LINEAGE_LINK_MAX = 4096                                     # members of a single-linkage component under complete or average linkage


def parse_lineage_link(text: str):
    """--lineage-link: single, complete or average -> vdjx_lineage_link_params.linkage; ValueError otherwise"""
    if text not in LINEAGE_LINKAGE:
        raise ValueError(f"--lineage-link must be single, complete or average: {text!r}")
    return LINEAGE_LINKAGE[text]


def junction_of(seq_id: str, contig: str):
    """junction_at of vdjer_main.c: the junction is the text after the id's second '_' (vjf_<n>_<junction>), looked for at its first
    occurrence in the contig -> (its 0-based start or -1, the text; '' when the id has none)"""
    parts = seq_id.split("_", 2)
    text = parts[2] if len(parts) == 3 else ""
    if not text or len(text) > len(contig):
        return -1, text
    return contig.find(text), text


def parse_lineage_dist(text: str):
    """--lineage-dist: a decimal in [0, 1] with at most four digits after the point, read exactly -> (num, 10000); ValueError otherwise
    (digits, at most one point, at least one digit: "0.15", ".2", "1", "1.", "1.0000"; no sign, no exponent, no blanks)"""
    whole, point, frac = text.partition(".")
    ok = bool(whole or frac) and len(whole) <= 1 and len(frac) <= 4 and all(ch in "0123456789" for ch in whole + frac)
    num = int(whole or "0") * 10000 + int((frac + "0000")[:4]) if ok else -1
    if not ok or num > 10000:
        raise ValueError(f"--lineage-dist must be a decimal in [0, 1] with at most four digits after the point: {text!r}")
    return num, 10000


def lineage_inputs(ids, contigs, v, j, names):
    """what `vdjer --lineages` hands to vdjx_lineage, from the V and the J hits ({field: array} as Context.annotate returns them) and the
    germline names -> (junctions, group uint32[n], vgene, jgene).  A contig is eligible when it has a V call and a J call (gene >= 0,
    both) and its junction is found in it with 3 .. 255 bases; its group is the index, by first appearance, of its distinct
    (vq_gene(V ties), vq_gene(J ties)) pair -- the strings --clones prints as vgene / jgene.  Every other contig gets LINEAGE_NONE and an
    empty junction; vgene / jgene are '' without a call."""
    import numpy as np
    n = len(ids)
    junctions, vgene, jgene = [], [], []
    group = np.full(n, LINEAGE_NONE, np.uint32)
    seen = {}
    for c in range(n):
        def gene(h):
            return vq_gene(names[g] for g in h["tied"][c][:min(8, int(h["n_tied"][c]))]) if h["gene"][c] >= 0 else ""
        vg, jg = gene(v), gene(j)
        p, text = junction_of(ids[c], contigs[c])
        ok = v["gene"][c] >= 0 and j["gene"][c] >= 0 and p >= 0 and 3 <= len(text) <= LINEAGE_MAXLEN
        if ok:
            group[c] = seen.setdefault((vg, jg), len(seen))
        junctions.append(text if ok else "")
        vgene.append(vg)
        jgene.append(jg)
    return junctions, group, vgene, jgene


def tree_inputs(ids, contigs, v, clone):
    """what `vdjer --trees` hands to vdjx_tree besides the contigs and the clones of the lineage step, from the V hits ({field: array} as
    Context.annotate returns them) -> (anchor int32[n], prio uint32[n]).  For a contig with clone >= 0 the anchor is where its junction
    starts (junction_of) and the priority its V hit's mismatches + ins + del: the member closest to its germline V becomes the root.
    Every other contig gets anchor 0 and priority 0."""
    import numpy as np
    n = len(ids)
    anchor, prio = np.zeros(n, np.int32), np.zeros(n, np.uint32)
    for c in range(n):
        if int(clone[c]) < 0:
            continue
        anchor[c] = junction_of(ids[c], contigs[c])[0]
        prio[c] = int(v["mismatches"][c]) + int(v["ins"][c]) + int(v["del"][c])
    return anchor, prio


def tree_nj_newick(ids, clone, parent, length, support=None, replicates=None):
    """the trees of Context.tree_nj as `vdjer --trees-newick` writes them: one string per lineage of two and more members, in ascending
    lineage number.  ids: the n contigs' names; clone: int32[n], the 0-based lineage number of every contig (-1: none), the clone given to
    tree_nj; parent, length: tree_nj's, [nodes].  The tree is rooted at the root member: (<its one subtree>)'<root id>'; -- children in
    ascending slot, every node labelled and single-quoted, 'label':%.4f of length / 65536; an inferred node is lin_<k>_a<j>, j from 1
    in creation order.  With support (Context.tree_split_support's, [nodes]) and replicates both given, a scored node (support >= 0) is
    labelled 'lin_<k>_a<j>/<%.4f of support / replicates>'; without them the strings are what they were.  Plain Python, no recursion: a
    lineage may be thousands of nodes deep."""
    n, nodes = len(ids), len(parent)
    if (support is None) != (replicates is None):
        raise ValueError("tree_nj_newick: support and replicates go together")
    if support is not None and (len(support) != nodes or int(replicates) < 1):
        raise ValueError(f"tree_nj_newick: support of {len(support)} entries for {nodes} nodes, {replicates} replicates")
    sizes = {}
    for k in clone:
        if int(k) >= 0:
            sizes[int(k)] = sizes.get(int(k), 0) + 1
    names = list(ids)
    for k in sorted(sizes):
        names += [f"lin_{k + 1}_a{j + 1}" for j in range(max(0, sizes[k] - 2))]
    if len(names) != nodes:
        raise ValueError(f"tree_nj_newick: {nodes} nodes, but the clones of the {n} contigs make {len(names)}")
    if support is not None:
        names = [f"{x}/%.4f" % (int(support[s]) / int(replicates)) if s >= n and int(support[s]) >= 0 else x for s, x in enumerate(names)]
    kids = [[] for _ in range(nodes)]
    for s in range(nodes):
        if int(parent[s]) >= 0:
            kids[int(parent[s])].append(s)
    roots = {int(clone[s]): s for s in range(n) if int(clone[s]) >= 0 and int(parent[s]) < 0}
    out = []
    for k in sorted(roots):
        if not kids[roots[k]]:
            continue
        text, stack = [], [(roots[k], 0)]
        while stack:
            s, at = stack.pop()
            if at == 0 and kids[s]:
                text.append("(")
            if at < len(kids[s]):
                if at:
                    text.append(",")
                stack.append((s, at + 1))
                stack.append((kids[s][at], 0))
                continue
            if kids[s]:
                text.append(")")
            text.append(f"'{names[s]}'" + ("" if s == roots[k] else ":%.4f" % (int(length[s]) / 65536)))
        out.append("".join(text) + ";")
    return out


def tree_split_compare(clone, parent_a, parent_b):
    """vdjx_tree_split_compare (plain C, no GPU): which splits of tree a tree b has.  clone: int32[n] as given to tree_nj; parent_a,
    parent_b: int32[nodes] in tree_nj's slots (tree_nj's and tree_mp's "parent", say) -> {"shared": int32[nodes] (1 or 0 for an inferred
    node of tree a other than a root's child, in a lineage of four and more; -1 elsewhere), "info": dict(shared, scored, rf)}; rf =
    2 (scored - shared) is the Robinson-Foulds distance of the two trees."""
    import ctypes as C

    import numpy as np

    from . import _lib
    cl = np.ascontiguousarray(clone, np.int32)
    pa, pb = np.ascontiguousarray(parent_a, np.int32), np.ascontiguousarray(parent_b, np.int32)
    if cl.ndim != 1 or pa.ndim != 1 or pb.shape != pa.shape:
        raise _lib.VdjxError(f"vdjx_tree_split_compare: clone of shape {cl.shape}, parents of shapes {pa.shape} and {pb.shape}")
    out = np.full(pa.shape[0], -1, np.int32)
    shared, scored = C.c_uint64(0), C.c_uint64(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.lib().vdjx_tree_split_compare(ptr(cl), cl.shape[0], ptr(pa), ptr(pb), pa.shape[0], ptr(out), C.byref(shared), C.byref(scored)),
               "vdjx_tree_split_compare")
    return {"shared": out, "info": {"shared": int(shared.value), "scored": int(scored.value), "rf": 2 * int(scored.value - shared.value)}}


def tree_mp_lengths(parent, mutations, clone):
    """the branch lengths `vdjer --trees-mp` and `--trees-mp-newick` print for Context.tree_mp's result, in tree_nj's unit of 1/65536:
    an edge's length is its mutations; 0 for a root, -1 for an item in no lineage.  tree_nj_newick takes them as they are."""
    import numpy as np
    parent, mutations, clone = (np.asarray(x) for x in (parent, mutations, clone))
    return np.where(clone < 0, -1, np.where(parent < 0, 0, mutations.astype(np.int64) << 16)).astype(np.int64)


def mutation_limit(ids, contigs):
    """the limit `vdjer --mutations` hands to vdjx_mutations -> int32[n]: V mutations are counted below the 0-based start of the junction
    (junction_of) plus 3, through the conserved Cys codon: what follows is the CDR3, where the germline row is not the V gene's to
    judge by.  The contig's length when the junction is not found."""
    import numpy as np
    out = np.zeros(len(ids), np.int32)
    for c, (cid, s) in enumerate(zip(ids, contigs)):
        p = junction_of(cid, s)[0]
        out[c] = min(p + 3, len(s)) if p >= 0 else len(s)
    return out


SELECTION_GRID = 4001                                       # VDJX_SEL_GRID (include/vdjx.h)


def selection_grid():
    """the grid of vdjx_selection's posterior -> float64[4001]: sigma_t = (t - 2000) / 100, -20 .. 20"""
    import numpy as np
    return (np.arange(SELECTION_GRID, dtype=np.float64) - 2000.0) / 100.0


def _whole(text: str, below: int):
    """the whole text as a decimal number below `below` (digits only, at least one), or None"""
    if not text or any(ch not in "0123456789" for ch in text) or len(text) > 20 or int(text) >= below:
        return None
    return int(text)


def read_v_regions(path: str, names, unmatched=None):
    """the region map of `vdjer --selection --v-regions` -> int32[records, 4] for vdjx_selection's cdr.  Lines `name cdr1_start cdr1_end
    cdr2_start cdr2_end`, separated by tabs or blanks; '#' lines and blank lines are skipped.  Positions are whole decimal numbers, 1-based
    and inclusive, 0 0 for no interval.  names: the records' names as parse_name gives them, in record order; every record of a line's name
    gets its intervals, a record without a line is -1 -1 -1 -1 (no regions).  A name that matches no record is appended to `unmatched`
    (when given).  ValueError, naming the line: not five fields, a position that is no whole number below 2^31, start > end, start 0 with
    end not 0, a name given twice."""
    import numpy as np
    out = np.full((len(names), 4), -1, np.int32)
    where = {}
    for r, nm in enumerate(names):
        where.setdefault(nm, []).append(r)
    seen = set()
    with open(path) as f:
        for no, line in enumerate(f, 1):
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            iv = [_whole(x, 1 << 31) for x in t[1:]]
            if len(t) != 5 or None in iv:
                raise ValueError(f"{path}: line {no}: expected `name cdr1_start cdr1_end cdr2_start cdr2_end` with whole numbers")
            for a, b in (iv[:2], iv[2:]):
                if a > b or (a == 0 and b != 0):
                    raise ValueError(f"{path}: line {no}: the interval {a} .. {b} (1 <= start <= end, or 0 0)")
            if t[0] in seen:
                raise ValueError(f"{path}: line {no}: the name {t[0]} is given twice")
            seen.add(t[0])
            if t[0] not in where:
                if unmatched is not None:
                    unmatched.append(t[0])
                continue
            for r in where[t[0]]:
                out[r] = iv
    return out


def read_targeting(path: str):
    """the targeting model of `vdjer --selection --targeting` -> uint32[1024, 4] for vdjx_selection's weight: row 256 a + 64 b + 16 c + 4 d +
    e of the 5-mer abcde (A 0, C 1, G 2, T 3), column the new base.  Exactly 1,024 lines `<5-mer> <wA> <wC> <wG> <wT>`, separated by tabs or
    blanks, each 5-mer over ACGT once; '#' lines and blank lines are skipped.  Weights are whole decimal numbers below 2^32 (the user scales
    the model, e.g. HH_S5F's targeting times 10^6); the column of the centre base is read and never used.  ValueError, naming the line."""
    import numpy as np
    out = np.zeros((1024, 4), np.uint32)
    seen = set()
    with open(path) as f:
        for no, line in enumerate(f, 1):
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            w = [_whole(x, 1 << 32) for x in t[1:]]
            if len(t) != 5 or None in w or len(t[0]) != 5 or any(ch not in "ACGT" for ch in t[0]):
                raise ValueError(f"{path}: line {no}: expected `<5-mer over ACGT> <wA> <wC> <wG> <wT>` with whole numbers below 2^32")
            idx = 0
            for ch in t[0]:
                idx = 4 * idx + "ACGT".index(ch)
            if idx in seen:
                raise ValueError(f"{path}: line {no}: the 5-mer {t[0]} is given twice")
            seen.add(idx)
            out[idx] = w
    if len(seen) != 1024:
        raise ValueError(f"{path}: {len(seen)} 5-mers, expected every one of the 1024 once")
    return out


def kmer5(m: int) -> str:
    """the 5-mer of row m of a targeting model: m = 256 a + 64 b + 16 c + 4 d + e"""
    return "".join("ACGT"[m >> s & 3] for s in (8, 6, 4, 2, 0))


def targeting_model(counts, cls="s", min_sub=50, min_mut=500):
    """vdjx_targeting_model (plain C, no GPU) over the uint64[2, 2, 1024, 4] counts of Context.targeting_counts -> (weight uint32[1024, 4]
    for vdjx_selection, level uint8[1024, 2]: the substitution and the mutability level 5, 3, 1 or 0 of every 5-mer).  cls: "s" (silent
    changes only) or "rs" (silent and replacement); min_sub, min_mut: whole numbers in 1 .. 2^32 - 1."""
    import ctypes as C

    import numpy as np

    from . import _lib
    counts = np.ascontiguousarray(counts, np.uint64)
    if counts.shape != (2, 2, 1024, 4):
        raise ValueError(f"counts of shape {counts.shape}, not (2, 2, 1024, 4)")
    if cls not in ("s", "rs"):
        raise ValueError(f"class {cls!r}: s or rs")
    for name, x in (("min_sub", min_sub), ("min_mut", min_mut)):
        if int(x) != x or not 1 <= int(x) < 1 << 32:
            raise ValueError(f"{name} = {x!r}: a whole number in 1 .. 2^32 - 1")
    weight, level = np.zeros((1024, 4), np.uint32), np.zeros((1024, 2), np.uint8)
    _lib.check(_lib.lib().vdjx_targeting_model(counts.ctypes.data_as(C.c_void_p), int(cls == "rs"), int(min_sub), int(min_mut),
                                               weight.ctypes.data_as(C.c_void_p), level.ctypes.data_as(C.c_void_p)), "vdjx_targeting_model")
    return weight, level


def write_targeting(path: str, weight, comments=()):
    """a targeting model as `vdjer --targeting-model` writes it and read_targeting / `vdjer --targeting` read it: the comments as '# '
    lines, then 1,024 lines `<5-mer>\\t<wA>\\t<wC>\\t<wG>\\t<wT>` in index order"""
    import numpy as np
    w = np.asarray(weight)
    if w.shape != (1024, 4) or (w < 0).any() or (w >= 1 << 32).any():
        raise ValueError(f"weights of shape {w.shape}: whole numbers below 2^32, [1024, 4]")
    with open(path, "w") as f:
        for line in comments:
            f.write(f"# {line}\n")
        for m in range(1024):
            f.write(kmer5(m) + "".join(f"\t{int(x)}" for x in w[m]) + "\n")


def lineage_distance_table(weight):
    """vdjx_lineage_distance_table (plain C, no GPU) over targeting weights -- uint32[1024, 4] as read_targeting returns them, or the path of
    such a file, read by read_targeting with its refusals -> (table uint16[1024, 4] for Context.lineage(table=...), info dict(mean,
    min_cost, max_cost)): -log10 of the targeting probability, normalised to a mean of 1, in thousandths; a centre cell is 0"""
    import ctypes as C

    import numpy as np

    from . import _lib
    if isinstance(weight, (str, bytes)) or hasattr(weight, "__fspath__"):
        weight = read_targeting(weight if isinstance(weight, str) else __import__("os").fsdecode(weight))
    given = np.asarray(weight)
    if given.shape != (1024, 4) or given.dtype.kind not in "ui" or (given < 0).any() or (given >= 1 << 32).any():
        raise ValueError(f"weights of shape {given.shape} and type {given.dtype}: whole numbers below 2^32, [1024, 4]")
    w = np.ascontiguousarray(given, np.uint32)
    table = np.zeros((1024, 4), np.uint16)
    info = _lib.LineageTableInfo()
    _lib.check(_lib.lib().vdjx_lineage_distance_table(w.ctypes.data_as(C.c_void_p), table.ctypes.data_as(C.c_void_p), C.byref(info)),
               "vdjx_lineage_distance_table")
    return table, dict(mean=float(info.mean), min_cost=int(info.min_cost), max_cost=int(info.max_cost))


def sankoff_costs(weight):
    """vdjx_sankoff_costs (plain C, no GPU) over targeting weights -- uint32[1024, 4] as read_targeting returns them, or the path of such a
    file -> (cost uint32[4, 4] for Context.tree_sankoff(cost=...), info dict(mean, min_cost, max_cost)): the 5-mer weights summed per centre
    base, -log10 of each substitution's share, normalised to a mean of 1, in thousandths; the diagonal is 0"""
    import ctypes as C

    import numpy as np

    from . import _lib
    if isinstance(weight, (str, bytes)) or hasattr(weight, "__fspath__"):
        weight = read_targeting(weight if isinstance(weight, str) else __import__("os").fsdecode(weight))
    given = np.asarray(weight)
    if given.shape != (1024, 4) or given.dtype.kind not in "ui" or (given < 0).any() or (given >= 1 << 32).any():
        raise ValueError(f"weights of shape {given.shape} and type {given.dtype}: whole numbers below 2^32, [1024, 4]")
    w = np.ascontiguousarray(given, np.uint32)
    cost = np.zeros((4, 4), np.uint32)
    info = _lib.SankoffCostsInfo()
    _lib.check(_lib.lib().vdjx_sankoff_costs(w.ctypes.data_as(C.c_void_p), cost.ctypes.data_as(C.c_void_p), C.byref(info)), "vdjx_sankoff_costs")
    return cost, dict(mean=float(info.mean), min_cost=int(info.min_cost), max_cost=int(info.max_cost))


THRESHOLD_GRID = 10000                                   # VDJX_THRESHOLD_GRID (include/vdjx.h): the grid is 0 .. 10000 ten-thousandths


def threshold_kernel(k):
    """vdjx_threshold_kernel (plain C, no GPU): the fixed-point Gaussian of bandwidth k / 1000, k = 1 .. 200 -> (uint32[10001]: w[d] =
    floor(2^30 exp(-d d / (200 k k)) + 0.5) up to its first 0 and zeros from there, len: the entries before that 0)"""
    import ctypes as C

    import numpy as np

    from . import _lib
    if not isinstance(k, (int, np.integer)) or not -(1 << 31) <= int(k) < 1 << 31:
        raise ValueError(f"a bandwidth k in 1 .. 200 thousandths, not {k!r}")
    w = np.zeros(THRESHOLD_GRID + 1, np.uint32)
    ln = C.c_uint32(0)
    _lib.check(_lib.lib().vdjx_threshold_kernel(int(k), w.ctypes.data_as(C.c_void_p), C.byref(ln)), "vdjx_threshold_kernel")
    return w, int(ln.value)


def threshold_bins(nearest, length, unit=1):
    """the bin rule of vdjx_lineage_threshold (include/vdjx.h) in plain Python integers -> int32[n]: the bin 0 .. 10000 of every item, -1
    for an item that takes no part (nearest -1; its length is not read): min(10000, (20000 nearest + unit L) // (2 unit L)).  ValueError
    where the library refuses: nearest below -1, a participating length of 0 or above 255, unit outside 1 .. 2^20, 2^20 items or more"""
    import numpy as np
    near, ln = [int(x) for x in nearest], [int(x) for x in length]
    if len(near) != len(ln) or len(near) >= 1 << 20:
        raise ValueError(f"{len(near)} nearest distances and {len(ln)} lengths: as many of each, fewer than 2^20")
    if not isinstance(unit, (int, np.integer)) or not 1 <= int(unit) <= 1 << 20:
        raise ValueError(f"unit {unit!r} (1 .. 2^20)")
    unit = int(unit)
    out = np.full(len(near), -1, np.int32)
    for i, (d, L) in enumerate(zip(near, ln)):
        if d < -1 or d >= 1 << 31:
            raise ValueError(f"item {i} has nearest {d} (-1: none)")
        if d < 0:
            continue
        if not 1 <= L <= 255:
            raise ValueError(f"item {i} has length {L} (1 .. 255)")
        out[i] = min(THRESHOLD_GRID, (2 * THRESHOLD_GRID * d + unit * L) // (2 * unit * L))
    return out


def _mix64(x):
    """splitmix64's output step, in 64-bit wrap-around arithmetic"""
    m = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ z >> 30) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ z >> 27) * 0x94D049BB133111EB) & m
    return z ^ z >> 31


def jackknife_keep(seed, r, w):
    """the keep rule of vdjx_tree_support (include/vdjx.h) in plain Python -> bool[w]: replicate r (1 .. replicates) keeps window position
    q when bit q & 31 of mix64(seed ^ (r << 32 | q >> 5)) is set"""
    import numpy as np
    seed, r = int(seed), int(r)
    assert 0 <= seed < 1 << 64 and 0 <= r < 1 << 32
    return np.array([bool(_mix64(seed ^ (r << 32 | q >> 5)) >> (q & 31) & 1) for q in range(int(w))], bool)


def diversity_orders():
    """the orders of `vdjer --diversity`: k / 10.0 for k = 0 .. 40 (q = 1.0 exactly at k = 10)"""
    return [k / 10.0 for k in range(41)]


def diversity_draw(seed, r, i, W):
    """the draw rule of vdjx_diversity (include/vdjx.h) in plain Python -> t in 0 .. W - 1: draw i (0 .. N - 1) of replicate r (1 ..
    replicates) is the high half of the 128-bit product mix64(mix64(seed) + (r << 32 | i)) * W; it falls on the clone k with
    cum[k] <= t < cum[k + 1]"""
    seed, r, i, W = int(seed), int(r), int(i), int(W)
    assert 0 <= seed < 1 << 64 and 0 <= r < 1 << 32 and 0 <= i < 1 << 32 and 0 <= W < 1 << 64
    return _mix64((_mix64(seed) + (r << 32 | i)) & ((1 << 64) - 1)) * W >> 64


def quant_boot_draw(seed, r, i, Pp):
    """the draw rule of vdjx_quant_boot (include/vdjx.h) in plain Python -> the slot in 0 .. Pp - 1 that draw i (0 .. Pp - 1) of replicate
    r (1 .. replicates) falls on: vdjx_diversity's rule with W = Pp, the placed pairs in ascending pair id being the slots"""
    return diversity_draw(seed, r, i, Pp)


def quant_boot_summary(boot):
    """vdjx_quant_boot_summary (plain C, no GPU) over a float64[B, n] matrix of replicate counts -> dict of float64[n]: mean, sd (n - 1;
    0 at B = 1), lower and upper (the 2.5 % and 97.5 % order statistics)"""
    import ctypes as C

    import numpy as np

    from . import _lib
    boot = np.ascontiguousarray(boot, np.float64)
    if boot.ndim != 2 or boot.shape[0] < 1:
        raise ValueError(f"a B x n matrix of replicate counts with B >= 1, not shape {boot.shape}")
    B, n = boot.shape
    out = {k: np.zeros(n, np.float64) for k in ("mean", "sd", "lower", "upper")}
    _lib.lib().vdjx_quant_boot_summary(boot.ctypes.data_as(C.c_void_p), B, n, *(out[k].ctypes.data_as(C.c_void_p) for k in ("mean", "sd", "lower", "upper")))
    return out


def selection_compare(pdf, pairs, skip=None):
    """vdjx_selection_compare (plain C, no GPU; shazam's testBaseline) over densities float64[rows, 4001] (any positive scale) and pairs
    [P, 2] of rows (a, b) -> dict of float64[P]: p_greater = P(sigma_a > sigma_b) + P(equal) / 2, pvalue = min(1, 2 min(p_greater,
    1 - p_greater)) and the Benjamini-Hochberg fdr over the pairs.  skip: None, or P flags; a flagged pair stays 0 and out of the fdr"""
    import ctypes as C

    import numpy as np

    from . import _lib
    pdf = np.ascontiguousarray(pdf, np.float64)
    if pdf.ndim != 2 or pdf.shape[1] != 4001:
        raise ValueError(f"densities of shape [rows, 4001], not {pdf.shape}")
    pr = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    P = pr.shape[0]
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    if sk is not None and sk.shape != (P,):
        raise ValueError(f"{P} pairs, skip of shape {sk.shape}")
    out = np.zeros((P, 3), np.float64)
    L = _lib.lib()
    rc = L.vdjx_selection_compare(pdf.ctypes.data_as(C.c_void_p), pdf.shape[0], pr.ctypes.data_as(C.c_void_p), P,
                                  None if sk is None else sk.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc:
        L.vdjx_last_error.restype = C.c_char_p
        raise ValueError(L.vdjx_last_error().decode())
    return {"p_greater": out[:, 0].copy(), "pvalue": out[:, 1].copy(), "fdr": out[:, 2].copy()}


def diversity_weights(clone, count_cells):
    """what `vdjer --diversity` hands to vdjx_diversity, from the lineage of every contig (Context.lineage's "clone"; -1: in none) and the
    printed expected_count cell of every contig ("12.34": two decimals, as the quant table has them) -> (uint64[C] weights, int list of
    the lineage numbers they belong to, ascending).  A lineage's weight is the sum of its members' cells read as integer hundredths,
    digit by digit, with no float; lineages of weight 0 and contigs in no lineage are left out."""
    import numpy as np
    sums = {}
    for k, cell in zip(clone, count_cells):
        k = int(k)
        if k < 0:
            continue
        whole, point, frac = str(cell).partition(".")
        if not (point and len(frac) == 2 and whole and all(ch in "0123456789" for ch in whole + frac)):
            raise ValueError(f"an expected_count cell has digits, a point and two digits: {cell!r}")
        w = 0
        for ch in whole + frac:
            w = w * 10 + (ord(ch) - 48)
        sums[k] = sums.get(k, 0) + w
    numbers = sorted(k for k, w in sums.items() if w > 0)
    return np.array([sums[k] for k in numbers], np.uint64), numbers


HIT_FIELDS = ("gene", "score", "n_tied", "tied", "seq_start", "seq_end", "germ_start", "germ_end", "matches", "mismatches", "ins", "del", "opens",
              "n_runs", "runs")
CONS_UNIT_FIELDS = ("group", "gene", "members", "off_record", "lo", "hi", "off")


def _hit_dtype():
    import numpy as np
    return np.dtype([(f, "<u4" if f == "runs" else "<i4", {"tied": (8,), "runs": (64,)}.get(f, ())) for f in HIT_FIELDS])      # vdjx_annot_hit


def _cons_unit_dtype():
    import numpy as np
    return np.dtype([(f, {"members": "<u4", "off_record": "<u4", "off": "<u8"}.get(f, "<i4")) for f in CONS_UNIT_FIELDS])       # vdjx_cons_unit


def consensus_layout(v, length, limit=None, group=None):
    """vdjx_consensus_layout (plain C, no GPU): the units of vdjx_consensus from the hits alone.  v: the field dict Context.annotate returns;
    length: the contigs' length; limit: int32[n] or None; group: int32[n] (negative: in no group) or None -> (unit int32[n]: the voter's
    unit or -1, {field: array[U]}: group, gene, members, off_record, lo, hi, off, the columns of all units together)"""
    import ctypes as C

    import numpy as np

    from . import _lib
    n = len(np.asarray(v["gene"]))
    hv = np.zeros(n, _hit_dtype())
    for f in HIT_FIELDS:
        hv[f] = np.asarray(v[f])
    lim = None if limit is None else np.ascontiguousarray(limit, np.int32)
    grp = None if group is None else np.ascontiguousarray(group, np.int32)
    if (lim is not None and lim.shape != (n,)) or (grp is not None and grp.shape != (n,)):
        raise ValueError(f"{n} hits, limit and group of as many entries")
    unit = np.full(n, -1, np.int32)
    units = np.zeros(max(n, 1), _cons_unit_dtype())
    nu, ncol = C.c_uint64(0), C.c_uint64(0)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.lib().vdjx_consensus_layout(ptr(hv), ptr(lim), ptr(grp), n, int(length), ptr(unit), ptr(units), C.byref(nu), C.byref(ncol)),
               "vdjx_consensus_layout")
    units = units[:int(nu.value)]
    return unit, {f: units[f].copy() for f in CONS_UNIT_FIELDS}, int(ncol.value)


def consensus_hits(units, cons, germ):
    """vdjx_consensus_hits (plain C, no GPU): the rows of Context.consensus as contigs and V hits that mutations(), selection() and
    targeting_counts() take.  units: {field: array[U]}; cons, germ: one str per unit -> (contigs: list[str] of one length -- a row without its
    '-', padded with N --, v: {field: array} of vdjx_annot_hit; a row without a base has gene -1 and score 0)"""
    import ctypes as C

    import numpy as np

    from . import _lib
    U = len(cons)
    if len(germ) != U or any(len(np.asarray(units[f])) != U for f in CONS_UNIT_FIELDS) or any(len(a) != len(b) for a, b in zip(cons, germ)):
        raise ValueError(f"{U} consensus rows, as many germline rows of the same lengths and as many units")
    un = np.zeros(max(U, 1), _cons_unit_dtype())
    for f in CONS_UNIT_FIELDS:
        un[f][:U] = np.asarray(units[f])
    off = 0
    for u in range(U):                                                # the rows as this call lays them out, whatever the units' own offsets were
        if len(cons[u]) != int(un["hi"][u]) - int(un["lo"][u]):
            raise ValueError(f"unit {u}: a row of {len(cons[u])} columns, positions {int(un['lo'][u])} .. {int(un['hi'][u])}")
        un["off"][u] = off
        off += len(cons[u])
    rc, rg = ("".join(cons).encode("latin-1") + b"\0"), ("".join(germ).encode("latin-1") + b"\0")
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    plen = C.c_int(0)
    L = _lib.lib()
    _lib.check(L.vdjx_consensus_hits(ptr(un), U, rc, rg, 0, None, None, C.byref(plen)), "vdjx_consensus_hits")
    pl = int(plen.value)
    text = np.zeros(max(U, 1) * pl, np.uint8)
    hv = np.zeros(max(U, 1), _hit_dtype())
    _lib.check(L.vdjx_consensus_hits(ptr(un), U, rc, rg, pl, ptr(text), ptr(hv), C.byref(plen)), "vdjx_consensus_hits")
    raw = text.tobytes()
    return [raw[u * pl:(u + 1) * pl].decode("latin-1") for u in range(U)], {f: hv[f][:U].copy() for f in HIT_FIELDS}
