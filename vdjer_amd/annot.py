"""Germline records for contig annotation (vdjx_germline_load, include/vdjx.h): the FASTA reader and the name / class rules that
`vdjer --airr` applies in C (vdjer_main.c) as well."""
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
