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
