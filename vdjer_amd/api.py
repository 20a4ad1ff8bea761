"""Host-side Python mirror of the C ABI in include/vdjx.h (one object per opaque handle).

The names follow the reference's call sites: a `Context` owns the V/J anchor sets
(vjf_init), the V-region index (score_seq_init) and the read index (add_read_info); `kmer_build`
stands where build_pre_graph/prune_pre_graph/build_graph2 stand in assemble() (A2:1388-1408);
`root_score` is score_seq (A2:1103); `window_score` is quick_map_process_contig + coverage_is_valid
(A2:841-847); `map_emit` is quick_map_process_contig_file (A2:912); `quant` is the RSEM step the reference's workflow runs
on vdjer.sam afterwards (demo/quant_demo.bash); `germline_load` / `annotate` stand for the IMGT HighV-QUEST run over
vdj_contigs.fa that the reference's post_process/collect_vdjer_stats.py reads.  `constant_load` / `isotype` stand for its isotype step
(call_isotypes.bash: STAR over the contigs' last 48 bases).
Everything computes on the GPU through libvdjx.so; nothing here falls back to a CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import CovParams, VdjxError, check

PAIR_DTYPE = np.dtype([("pair_id", "<u4"), ("rec1", "<u4"), ("rec2", "<u4"), ("pos1", "<i2"), ("pos2", "<i2"),
                       ("insert", "<i2"), ("rc1", "u1"), ("rc2", "u1")])
assert PAIR_DTYPE.itemsize == C.sizeof(_lib.Pair)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


@dataclass
class Graph:
    """Result of kmer_build: nodes in creation order + ordered edge lists (1-based ids, list order)."""
    k: int
    n: int
    pre_nodes: int
    first_inst: np.ndarray
    gated_count: np.ndarray
    freq: np.ndarray
    has_v: np.ndarray
    has_j: np.ndarray
    to_deg: np.ndarray
    to_ids: np.ndarray
    from_deg: np.ndarray
    from_ids: np.ndarray
    kmers: np.ndarray        # [n, k] uint8 ASCII
    n_roots: int = 0
    handle: object = None    # the device-resident graph (kept only with keep_device=True); free() releases it
    ctx: object = None

    def kmer(self, i: int) -> str:
        return self.kmers[i].tobytes().decode()

    def wait(self):
        """after kmer_build(..., async_export=True): the host arrays are valid once this returns"""
        if self.handle is not None and getattr(self, "_pending", False):
            check(_lib.lib().vdjx_graph_export_end(self.handle), "vdjx_graph_export_end")
            self._pending = False

    def free(self):
        if self.handle is not None:
            self.wait()
            _lib.lib().vdjx_graph_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Pool:
    def __init__(self, ctx: "Context", handle, rl: int, n_records: int):
        self.ctx, self.h, self.rl, self.n_records = ctx, handle, rl, n_records
        self._src = None           # host buffers an asynchronous load still reads

    def wait(self):
        """after pool_load_forward(..., wait=False): the pool is loaded (and well-formed) once this returns"""
        try:
            check(_lib.lib().vdjx_pool_wait(self.h), "vdjx_pool_wait")
        finally:
            self._src = None

    def free(self):
        if self.h:
            _lib.lib().vdjx_pool_free(self.h)      # (waits for a load that is still running)
            self.h = None
            self._src = None
            if self in getattr(self.ctx, "_pools", []):
                self.ctx._pools.remove(self)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """pinned_results=True: result arrays (graph export, mapped pairs) are views of page-locked buffers owned by the context
    and REUSED by the next call of the same kind — the way a C caller keeps one set of result buffers per stage."""

    def __init__(self, device: int = 0, pinned_results: bool = False):
        self.L = _lib.lib()
        h = C.c_void_p()
        check(self.L.vdjx_init(device, C.byref(h)), "vdjx_init")
        self.h = h
        self.device = device
        self._pools = []
        self.pinned_results = pinned_results
        self._pinned = {}            # tag -> (ptr, capacity bytes)
        self._retired = []           # outgrown pinned buffers, freed with the context

    def _result_arrays(self, tag: str, specs):
        """specs: [(shape, dtype)] -> zero-copy numpy arrays; pinned and recycled per `tag` when pinned_results is set"""
        if not self.pinned_results:
            return [np.zeros(shape, dt) for shape, dt in specs]
        sizes = [int(np.prod(shape)) * np.dtype(dt).itemsize for shape, dt in specs]
        need = sum((b + 255) & ~255 for b in sizes) + 256
        ptr, cap = self._pinned.get(tag, (None, 0))
        if cap < need:
            if ptr:
                # arrays of an earlier result may still be views of the old buffer (and an asynchronous export may still be
                # writing into it): it is retired, not freed, until the context closes
                self._retired.append(ptr)
            new = C.c_void_p()
            cap = need + need // 4
            check(self.L.vdjx_host_alloc(self.h, cap, C.byref(new)), "vdjx_host_alloc")
            ptr = new.value
            self._pinned[tag] = (ptr, cap)
        # (the views of the last call with the same shapes over the same buffer are the same arrays: building ten of them costs ~0.1 ms,
        # a tenth of a whole step on a small pool)
        key = (ptr, tuple((tuple(shape), np.dtype(dt).str) for shape, dt in specs))
        views = getattr(self, "_views", None)
        if views is None:
            views = self._views = {}
        hit = views.get(tag)
        if hit is not None and hit[0] == key:
            return list(hit[1])
        out, at = [], ptr
        for (shape, dt), b in zip(specs, sizes):
            raw = (C.c_uint8 * max(b, 1)).from_address(at)
            out.append(np.frombuffer(raw, dtype=dt, count=int(np.prod(shape))).reshape(shape))
            at += (b + 255) & ~255
        views[tag] = (key, list(out))
        return out

    def close(self):
        for p in list(getattr(self, "_pools", [])):
            p.free()
        self._pools = []
        if getattr(self, "h", None):
            for ptr, _ in getattr(self, "_pinned", {}).values():
                self.L.vdjx_host_free(self.h, ptr)
            for ptr in getattr(self, "_retired", []):
                self.L.vdjx_host_free(self.h, ptr)
            self._pinned, self._retired = {}, []
            self.L.vdjx_shutdown(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.L.vdjx_sync(self.h), "vdjx_sync")

    def device_copy(self, d_dst: int, d_src: int, nbytes: int) -> None:
        check(self.L.vdjx_device_copy(self.h, C.c_void_p(d_dst), C.c_void_p(d_src), nbytes), "vdjx_device_copy")

    def read_index_drop(self):
        check(self.L.vdjx_read_index_drop(self.h), "vdjx_read_index_drop")

    def trim(self):
        """hand the workspaces' device memory back (vdjx_trim): a context keeps the peak of its calls otherwise"""
        check(self.L.vdjx_trim(self.h), "vdjx_trim")

    # ---- a-0
    def pool_load(self, primary: np.ndarray, secondary: np.ndarray, rl: int) -> Pool:
        pri = _c(primary, np.uint8).reshape(-1, 2 * rl + 1)
        sec = _c(secondary, np.uint8).reshape(-1, 2 * rl + 1)
        h = C.c_void_p()
        check(self.L.vdjx_pool_load(self.h, _p(pri), pri.shape[0], _p(sec), sec.shape[0], rl, C.byref(h)), "vdjx_pool_load")
        p = Pool(self, h, rl, pri.shape[0] + sec.shape[0])
        self._pools.append(p)
        return p

    @staticmethod
    def packed_read_bytes(rl: int) -> int:
        return int(_lib.lib().vdjx_packed_read_bytes(rl))

    @staticmethod
    def pack_reads(ascii_reads: np.ndarray, rl: int) -> np.ndarray:
        """[n, 2*rl+1] ASCII records of reads ('0' + bases + qualities) -> [n, packed_read_bytes(rl)] in the packed host format
        (vdjx_pack_reads: 2-bit bases, then the quality bytes with bit 7 = not ACGT)"""
        a = _c(ascii_reads, np.uint8).reshape(-1, 2 * rl + 1)
        S = Context.packed_read_bytes(rl)
        out = np.zeros((a.shape[0], S), np.uint8)
        check(_lib.lib().vdjx_pack_reads(_p(a), a.shape[0], rl, _p(out)), "vdjx_pack_reads")
        return out

    def pool_load_packed(self, primary_reads, secondary_reads, rl: int, n_primary: int = None, n_secondary: int = None, wait: bool = True) -> Pool:
        """pool_load_forward for reads in the packed host format ([n, packed_read_bytes(rl)] uint8 arrays, or raw host addresses with counts)"""
        S = self.packed_read_bytes(rl)
        if isinstance(primary_reads, int):
            pp, ps, npri, nsec = C.c_void_p(primary_reads), C.c_void_p(secondary_reads), n_primary, n_secondary
        else:
            pri = _c(primary_reads, np.uint8).reshape(-1, S)
            sec = _c(secondary_reads, np.uint8).reshape(-1, S)
            pp, ps, npri, nsec = _p(pri), _p(sec), pri.shape[0], sec.shape[0]
        h = C.c_void_p()
        fn = self.L.vdjx_pool_load_packed if wait else self.L.vdjx_pool_load_packed_begin
        check(fn(self.h, pp, npri, ps, nsec, rl, C.byref(h)), "vdjx_pool_load_packed")
        p = Pool(self, h, rl, 2 * (npri + nsec))
        if not wait and not isinstance(primary_reads, int):
            p._src = (pri, sec)
        self._pools.append(p)
        return p

    def pool_load_forward(self, primary_reads, secondary_reads, rl: int, n_primary: int = None, n_secondary: int = None,
                          wait: bool = True) -> Pool:
        """the reads as extracted only ([n, 2*rl+1] uint8 arrays or raw host addresses with counts): every read's reverse-complement
        record is derived on the device (record 2i = read i, 2i+1 = its reverse complement)"""
        if isinstance(primary_reads, int):
            pp, ps, npri, nsec = C.c_void_p(primary_reads), C.c_void_p(secondary_reads), n_primary, n_secondary
        else:
            pri = _c(primary_reads, np.uint8).reshape(-1, 2 * rl + 1)
            sec = _c(secondary_reads, np.uint8).reshape(-1, 2 * rl + 1)
            pp, ps, npri, nsec = _p(pri), _p(sec), pri.shape[0], sec.shape[0]
        h = C.c_void_p()
        fn = self.L.vdjx_pool_load_forward if wait else self.L.vdjx_pool_load_forward_begin      # wait=False: Pool.wait() before use
        check(fn(self.h, pp, npri, ps, nsec, rl, C.byref(h)), "vdjx_pool_load_forward")
        p = Pool(self, h, rl, 2 * (npri + nsec))
        if not wait and not isinstance(primary_reads, int):
            # the upload is still reading these buffers (they may be contiguous COPIES made above): the pool keeps them alive
            # until Pool.wait() / free()
            p._src = (pri, sec)
        self._pools.append(p)
        return p

    def pool_load_device(self, d_primary, n_primary: int = None, d_secondary=None, n_secondary: int = None, rl: int = None, keepalive=None) -> Pool:
        """ASCII pools already resident in device memory (16-byte aligned).

        LIFETIME (include/vdjx.h, vdjx_pool_load_device): bases and masks are packed, but the quality characters are NOT copied --
        the pool keeps pointers into the two buffers, which must stay valid and unchanged until Pool.free().  Pass the buffers as
        torch tensors ([records, 2*rl+1] uint8, contiguous) and the Pool holds references to them until it is freed; with raw
        device pointers (ints) the caller answers for the lifetime, or hands the owning objects over in `keepalive`.  A buffer
        that is released or overwritten while the pool lives gives silently wrong quality sums and SAM qualities."""
        owners = [keepalive] if keepalive is not None else []

        def as_ptr(x, n):
            if hasattr(x, "data_ptr"):
                if not x.is_contiguous():
                    raise VdjxError("vdjx_pool_load_device: the buffer must be contiguous")
                owners.append(x)
                return x.data_ptr(), (int(x.shape[0]) if n is None else n), (int(x.shape[1] - 1) // 2 if x.dim() == 2 else None)
            return (int(x) if x is not None else 0), (n or 0), None
        pp, np_, rl_p = as_ptr(d_primary, n_primary)
        ps, ns_, rl_s = as_ptr(d_secondary, n_secondary)
        if rl is None:
            rl = rl_p if rl_p is not None else rl_s
        if rl is None:
            raise VdjxError("vdjx_pool_load_device: rl is needed with raw pointers")
        h = C.c_void_p()
        check(self.L.vdjx_pool_load_device(self.h, C.c_void_p(pp), np_, C.c_void_p(ps), ns_, rl, C.byref(h)), "vdjx_pool_load_device")
        p = Pool(self, h, rl, np_ + ns_)
        p._src = owners or None      # dropped in Pool.free()
        self._pools.append(p)
        return p

    # ---- a-6
    def anchor_sets_load(self, v_codes, j_codes) -> None:
        v = _c(v_codes, np.uint32)
        j = _c(j_codes, np.uint32)
        check(self.L.vdjx_anchor_sets_load(self.h, _p(v), v.shape[0], _p(j), j.shape[0]), "vdjx_anchor_sets_load")

    def anchor_sets_from_anchors(self, v_anchor_codes, j_anchor_codes, am: int = 4) -> None:
        """the sets of anchor_sets_load, built on the device from the anchors themselves (Hamming balls of radius min(am, 5))"""
        v, j = _c(v_anchor_codes, np.uint32), _c(j_anchor_codes, np.uint32)
        check(self.L.vdjx_anchor_sets_from_anchors(self.h, _p(v), v.shape[0], _p(j), j.shape[0], am), "vdjx_anchor_sets_from_anchors")

    def index_generate(self, anchor_codes, start: int = 0, end: int = 2 ** 32 - 1, max_dist: int = 5):
        """rows of a v_index / j_index file (seq_dist.c:49-71) for the codes [start, end]: (codes uint32, distances uint8)"""
        a = _c(anchor_codes, np.uint32)
        n = C.c_uint64()
        check(self.L.vdjx_index_generate(self.h, _p(a), a.shape[0], start, end, max_dist, 0, C.byref(n), None, None), "vdjx_index_generate(count)")
        codes, dists = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint8)
        if n.value:
            check(self.L.vdjx_index_generate(self.h, _p(a), a.shape[0], start, end, max_dist, n.value, C.byref(n), _p(codes), _p(dists)),
                  "vdjx_index_generate")
        return codes, dists

    def anchor_probe(self, contig: str):
        n = max(0, len(contig) - 16)
        ov = np.zeros(n, np.uint8)
        oj = np.zeros(n, np.uint8)
        check(self.L.vdjx_anchor_probe(self.h, contig.encode(), len(contig), _p(ov), _p(oj)), "vdjx_anchor_probe")
        return ov, oj

    # ---- a-1..a-3
    def kmer_build(self, pool: Pool, k: int = 35, mf: int = 3, mq: int = 90, export: bool = True, keep_device: bool = False,
                   async_export: bool = False):
        """async_export (implies keep_device): the copy of the graph into the host arrays runs on a second stream beside whatever
        is done next with the context; call Graph.wait() before reading the arrays"""
        g = C.c_void_p()
        check(self.L.vdjx_kmer_build(self.h, pool.h, k, mf, mq, C.byref(g)), "vdjx_kmer_build")
        if not export:
            try:
                return int(self.L.vdjx_graph_nodes(g)), int(self.L.vdjx_graph_pre_nodes(g))
            finally:
                self.L.vdjx_graph_free(g)
        return self._export_graph(g, k, keep_device or async_export, async_export)

    def _export_graph(self, g, k: int, keep_device: bool = False, async_export: bool = False) -> Graph:
        """copy a finished graph into host arrays; the handle is released unless keep_device (then Graph.free() does it)"""
        keep = False
        try:
            n = int(self.L.vdjx_graph_nodes(g))
            if self.pinned_results and n:
                # ONE transfer of the graph's device block into a page-locked block of the same layout; the arrays are views of it
                # (ten transfers cost a small pool's step a tenth of its time in calls alone)
                offs, nb = (C.c_uint64 * 10)(), C.c_uint64()
                check(self.L.vdjx_graph_block_layout(g, offs, C.byref(nb)), "vdjx_graph_block_layout")
                blk = self._result_arrays("graphblock", [((int(nb.value),), np.uint8)])[0]
                key = (blk.ctypes.data, n, k, tuple(offs))
                hit = getattr(self, "_graph_views", None)
                if hit is None or hit[0] != key:
                    specs = [(np.uint64, (n,)), (np.uint32, (n,)), (np.uint32, (n,)), (np.uint8, (n,)), (np.uint8, (n,)), (np.uint8, (n,)),
                             (np.uint32, (n, 4)), (np.uint8, (n,)), (np.uint32, (n, 4)), (np.uint8, (n, k))]
                    views = [blk[int(o):int(o) + int(np.prod(sh)) * np.dtype(dt).itemsize].view(dt).reshape(sh) for o, (dt, sh) in zip(offs, specs)]
                    hit = self._graph_views = (key, views)
                out = Graph(k, n, int(self.L.vdjx_graph_pre_nodes(g)), *hit[1], n_roots=int(self.L.vdjx_graph_roots(g)))
                fn = self.L.vdjx_graph_export_block_begin if async_export else self.L.vdjx_graph_export_block
                check(fn(g, _p(blk)), "vdjx_graph_export_block")
                if keep_device:
                    out.handle, out.ctx, keep = g, self, True
                    out._pending = async_export
                return out
            out = Graph(k, n, int(self.L.vdjx_graph_pre_nodes(g)), *self._result_arrays("graph", [
                ((n,), np.uint64), ((n,), np.uint32), ((n,), np.uint32), ((n,), np.uint8), ((n,), np.uint8), ((n,), np.uint8),
                ((n, 4), np.uint32), ((n,), np.uint8), ((n, 4), np.uint32), ((n, k), np.uint8)]),
                n_roots=int(self.L.vdjx_graph_roots(g)))
            fn = self.L.vdjx_graph_export_begin if async_export else self.L.vdjx_graph_export
            check(fn(g, _p(out.first_inst), _p(out.gated_count), _p(out.freq), _p(out.has_v), _p(out.has_j), _p(out.to_deg),
                     _p(out.to_ids), _p(out.from_deg), _p(out.from_ids), _p(out.kmers)), "vdjx_graph_export")
            if keep_device:
                out.handle, out.ctx, keep = g, self, True
                out._pending = async_export
            return out
        finally:
            if not keep:
                self.L.vdjx_graph_free(g)

    # ---- a-7
    def vregion_load(self, lines, vk: int = 15) -> None:
        arr = (C.c_char_p * len(lines))(*[s.encode() for s in lines])
        check(self.L.vdjx_vregion_load(self.h, arr, len(lines), vk), "vdjx_vregion_load")

    def root_score(self, kmers, k: int, threshold: int) -> np.ndarray:
        if isinstance(kmers, np.ndarray):
            buf = _c(kmers, np.uint8).reshape(-1, k)
            n = buf.shape[0]
            raw = buf.tobytes()
        else:
            n = len(kmers)
            raw = "".join(kmers).encode()
            assert len(raw) == n * k
        out = np.zeros(n, np.uint8)
        check(self.L.vdjx_root_score(self.h, raw, n, k, threshold, _p(out)), "vdjx_root_score")
        return out

    def root_score_graph(self, graph: Graph, threshold: int, first: int = 0, stride: int = 1, wait: bool = True):
        """scores the roots of a device-resident graph (kmer_build(..., keep_device=True)): (1-based node ids, verdicts).
        On a context made with pinned_results=True the two arrays are views of ONE recycled page-locked buffer (like every pinned
        result of this class): they are valid until the next root_score_graph call of the context -- a second call of the same size
        returns the very same arrays with new contents.  Copy them (np.array(x)) to hold two results at once."""
        if graph.handle is None:
            raise VdjxError("root_score_graph: the graph was not kept on the device (keep_device=True)")
        n = int(self.L.vdjx_root_part(graph.handle, first, stride))
        ids, out = self._result_arrays("roots", [((n,), np.uint32), ((n,), np.uint8)])
        if not wait and self.pinned_results:
            # queued, not waited for: the arrays are valid after root_score_wait() (vdjx_root_score_graph_begin / _end)
            check(self.L.vdjx_root_score_graph_begin(self.h, graph.handle, threshold, first, stride, _p(ids), _p(out)), "vdjx_root_score_graph_begin")
            self._roots_pending = True
            return ids, out
        check(self.L.vdjx_root_score_graph(self.h, graph.handle, threshold, first, stride, _p(ids), _p(out)), "vdjx_root_score_graph")
        return ids, out

    def root_score_wait(self):
        if getattr(self, "_roots_pending", False):
            self._roots_pending = False
            check(self.L.vdjx_root_score_graph_end(self.h), "vdjx_root_score_graph_end")

    # ---- a-8..a-10
    def read_index_build(self, pool: Pool, pair_id, read_num, is_rc, reg_rank, n_pairs: int) -> None:
        a, b, c_, d = _c(pair_id, np.uint32), _c(read_num, np.uint8), _c(is_rc, np.uint8), _c(reg_rank, np.uint32)
        assert a.shape[0] == pool.n_records
        check(self.L.vdjx_read_index_build(self.h, pool.h, _p(a), _p(b), _p(c_), _p(d), n_pairs), "vdjx_read_index_build")

    def read_index_build_device(self, pool: Pool, d_pair_id: int, d_read_num: int, d_is_rc: int, d_reg_rank: int, n_pairs: int, wait: bool = True) -> None:
        """the per-record arrays as raw device pointers (uint32, uint8, uint8, uint32; one entry per pool record).
        wait=False: begun on the index stream, beside the calls that follow (the k-mer build of the same pool); read_index_wait() --
        or the first scorer call -- ends it (vdjx_read_index_build_device_begin / _end)"""
        if not wait:
            check(self.L.vdjx_read_index_build_device_begin(self.h, pool.h, C.c_void_p(d_pair_id), C.c_void_p(d_read_num), C.c_void_p(d_is_rc),
                                                            C.c_void_p(d_reg_rank), n_pairs), "vdjx_read_index_build_device_begin")
            return
        check(self.L.vdjx_read_index_build_device(self.h, pool.h, C.c_void_p(d_pair_id), C.c_void_p(d_read_num), C.c_void_p(d_is_rc),
                                                  C.c_void_p(d_reg_rank), n_pairs), "vdjx_read_index_build_device")

    def read_index_build_begin(self, pool: Pool, pair_id, read_num, is_rc, reg_rank, n_pairs: int) -> None:
        """host arrays, begun (vdjx_read_index_build_begin): they are kept alive here until read_index_wait()"""
        a, b, c_, d = _c(pair_id, np.uint32), _c(read_num, np.uint8), _c(is_rc, np.uint8), _c(reg_rank, np.uint32)
        assert a.shape[0] == pool.n_records
        self._ri_keep = (a, b, c_, d, pool)
        check(self.L.vdjx_read_index_build_begin(self.h, pool.h, _p(a), _p(b), _p(c_), _p(d), n_pairs), "vdjx_read_index_build_begin")

    def read_index_wait(self) -> None:
        try:
            check(self.L.vdjx_read_index_build_end(self.h), "vdjx_read_index_build_end")
        finally:
            self._ri_keep = None

    @staticmethod
    def pack_strings(strings):
        """(raw bytes, n, len) of equally long strings: pass it instead of the list to skip the per-call join/encode"""
        n = len(strings)
        ln = len(strings[0]) if n else 0
        assert all(len(w) == ln for w in strings)
        return ("".join(strings).encode(), n, ln)

    def pin_strings(self, strings, tag: str):
        """pack_strings into a page-locked buffer owned by the context (one per `tag`): the scorers' input then crosses PCIe as a
        DMA instead of being staged by the runtime (a C caller builds its windows in vdjx_host_alloc memory to the same effect)"""
        raw, n, ln = self.pack_strings(strings)
        need = max(len(raw), 1)
        ptr, cap = self._pinned.get("in:" + tag, (None, 0))
        if cap < need:
            if ptr:
                self._retired.append(ptr)
            new = C.c_void_p()
            check(self.L.vdjx_host_alloc(self.h, need, C.byref(new)), "vdjx_host_alloc")
            ptr, cap = new.value, need
            self._pinned["in:" + tag] = (ptr, cap)
        C.memmove(ptr, raw, len(raw))
        return (C.cast(ptr, C.c_char_p), n, ln)

    def pin_array(self, rows: np.ndarray, tag: str):
        """pin_strings for strings that already are the rows of a C-contiguous uint8 matrix (no join / encode)"""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        n, ln = rows.shape
        need = max(rows.nbytes, 1)
        ptr, cap = self._pinned.get("in:" + tag, (None, 0))
        if cap < need:
            if ptr:
                self._retired.append(ptr)
            new = C.c_void_p()
            check(self.L.vdjx_host_alloc(self.h, need + need // 4, C.byref(new)), "vdjx_host_alloc")
            ptr, cap = new.value, need + need // 4
            self._pinned["in:" + tag] = (ptr, cap)
        C.memmove(ptr, rows.ctypes.data, rows.nbytes)
        return (C.cast(ptr, C.c_char_p), n, ln)

    def pin_rows_take(self, rows: np.ndarray, idx: np.ndarray, tag: str, first: int = 0, length: int | None = None):
        """pin_array(rows[idx, first:first + length]) without intermediate arrays: the chosen rows' slices are copied straight into
        the page-locked buffer (vdjx_host_take_rows)"""
        assert rows.dtype == np.uint8 and rows.ndim == 2 and rows.flags.c_contiguous
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        n = int(idx.shape[0])
        ln = int(rows.shape[1]) - first if length is None else int(length)
        need = max(n * ln, 1)
        ptr, cap = self._pinned.get("in:" + tag, (None, 0))
        if cap < need:
            if ptr:
                self._retired.append(ptr)
            new = C.c_void_p()
            check(self.L.vdjx_host_alloc(self.h, need + need // 4, C.byref(new)), "vdjx_host_alloc")
            ptr, cap = new.value, need + need // 4
            self._pinned["in:" + tag] = (ptr, cap)
        if n and int(idx.max()) >= rows.shape[0]:
            raise IndexError("pin_rows_take: row index out of range")
        check(self.L.vdjx_host_take_rows(ptr, rows.ctypes.data, rows.shape[1], first, ln, idx.ctypes.data, n), "vdjx_host_take_rows")
        return (C.cast(ptr, C.c_char_p), n, ln)

    def window_score(self, windows, ins: int, e0: int = 52, e1: int = 411, rs: int = 35, ms: int = 48, floor: int = 1):
        raw, n, ln = windows if isinstance(windows, tuple) else self.pack_strings(windows)
        if n == 0:
            return np.zeros(0, np.uint8), np.zeros(0, np.uint32)
        cp = CovParams(e0, e1, rs, ms, ins, ins, floor)
        valid = np.zeros(n, np.uint8)
        npairs = np.zeros(n, np.uint32)
        check(self.L.vdjx_window_score(self.h, raw, n, ln, C.byref(cp), _p(valid), _p(npairs)), "vdjx_window_score")
        return valid, npairs

    # ---- the halves of window_score for a pool sharded by pair over several GPUs (vdjer_amd/shard.py drives them)
    def window_pairs(self, windows):
        """-> (entries per window's pair list, mapped pairs per window); the lists stay on the device for window_pairs_fetch"""
        raw, n, ln = windows if isinstance(windows, tuple) else self.pack_strings(windows)
        ent, npairs = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        if n:
            check(self.L.vdjx_window_pairs(self.h, raw, n, ln, _p(ent), _p(npairs)), "vdjx_window_pairs")
        return ent, npairs

    def window_pairs_fetch(self, window_ids, d_out: int):
        ids = _c(window_ids, np.uint32)
        check(self.L.vdjx_window_pairs_fetch(self.h, _p(ids), ids.shape[0], C.c_void_p(d_out)), "vdjx_window_pairs_fetch")

    def window_cover(self, n: int, ln: int, rl: int, d_lists: int, nsrc: int, counts, ins: int, e0: int = 52, e1: int = 411, rs: int = 35,
                     ms: int = 48, floor: int = 1, ins_high: int | None = None) -> np.ndarray:
        """counts [nsrc, n] (source-major) entries per source and window; d_lists: device pointer to the lists in that order.
        ins_high: insert_high where it differs from insert_low (= ins)"""
        cnt = _c(counts, np.uint32).reshape(-1)
        assert cnt.shape[0] == nsrc * n
        cp = CovParams(e0, e1, rs, ms, ins, ins if ins_high is None else ins_high, floor)
        valid = np.zeros(n, np.uint8)
        if n:
            check(self.L.vdjx_window_cover(self.h, n, ln, rl, C.byref(cp), C.c_void_p(d_lists), nsrc, _p(cnt), _p(valid)), "vdjx_window_cover")
        return valid

    def map_emit(self, contigs, async_copy: bool = False):
        """async_copy: the pairs travel to the host on the copy stream while the caller goes on (two alternating pinned result
        buffers); they are valid after map_emit_wait(), which the next map_emit call also performs"""
        raw, n, ln = contigs if isinstance(contigs, tuple) else self.pack_strings(contigs)
        offs = np.zeros(n + 1, np.uint64)
        if n == 0:
            return offs, np.zeros(0, PAIR_DTYPE)
        self.map_emit_wait()
        check(self.L.vdjx_map_emit(self.h, raw, n, ln, _p(offs), None), "vdjx_map_emit(count)")
        self._pairs_flip = 1 - getattr(self, "_pairs_flip", 0)
        pairs, = self._result_arrays(f"pairs{self._pairs_flip}" if async_copy else "pairs", [((int(offs[n]),), PAIR_DTYPE)])
        if async_copy:
            check(self.L.vdjx_map_emit_begin(self.h, raw, n, ln, _p(offs), _p(pairs)), "vdjx_map_emit_begin")
            self._pairs_pending = True
        else:
            check(self.L.vdjx_map_emit(self.h, raw, n, ln, _p(offs), _p(pairs)), "vdjx_map_emit")
        return offs, pairs

    def map_emit_wait(self):
        if getattr(self, "_pairs_pending", False):
            check(self.L.vdjx_map_emit_end(self.h), "vdjx_map_emit_end")
            self._pairs_pending = False

    def sam_names_load(self, names) -> None:
        """read names by pair id (list of str) for sam_text_device"""
        enc = [s_.encode() for s_ in names]
        off = np.zeros(len(enc) + 1, np.uint64)
        off[1:] = np.cumsum([len(e) for e in enc])
        check(self.L.vdjx_sam_names_load(self.h, b"".join(enc), _p(off), len(enc)), "vdjx_sam_names_load")

    def sam_names_load_raw(self, cat: np.ndarray, off: np.ndarray) -> None:
        """the same from the names laid end to end (uint8) and their offsets (uint64 [n_pairs + 1]): no Python string per pair"""
        cat = np.ascontiguousarray(cat, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        check(self.L.vdjx_sam_names_load(self.h, C.cast(cat.ctypes.data, C.c_char_p), _p(off), off.shape[0] - 1), "vdjx_sam_names_load")

    @staticmethod
    def _ids(contig_ids, n):
        enc = [s_.encode() for s_ in contig_ids]
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum([len(e) for e in enc])
        return b"".join(enc), off

    def sam_blocks(self, contigs, contig_ids, d_reg_rank: int):
        """vdjx_sam_blocks: the SAM records of THIS context's pairs for these contigs (a pool sharded by pair), left on the device:
        -> (blocks, bytes, d_keys, d_lens, d_text) -- device pointers owned by the context, valid until the next sam_blocks / sam_text.
        d_reg_rank: device pointer, the GLOBAL registration rank of every record of the index's pool."""
        raw, n, ln = contigs if isinstance(contigs, tuple) else self.pack_strings(contigs)
        ids, off = self._ids(contig_ids, n)
        nb, nby = C.c_uint64(), C.c_uint64()
        dk, dl, dt = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self.L.vdjx_sam_blocks(self.h, raw, n, ln, ids, _p(off), C.c_void_p(d_reg_rank), C.byref(nb), C.byref(nby), C.byref(dk), C.byref(dl), C.byref(dt)),
              "vdjx_sam_blocks")
        return int(nb.value), int(nby.value), dk.value or 0, dl.value or 0, dt.value or 0

    def sam_merge(self, n_blocks: int, n_bytes: int, d_keys: int, d_lens: int, d_text: int) -> bytes:
        """vdjx_sam_merge: the blocks of all sources (source after source) laid out in ascending key order = the reference's order"""
        txt, nb = C.c_char_p(), C.c_uint64()
        check(self.L.vdjx_sam_merge(self.h, n_blocks, n_bytes, C.c_void_p(d_keys), C.c_void_p(d_lens), C.c_void_p(d_text), C.byref(txt), C.byref(nb)), "vdjx_sam_merge")
        addr = C.cast(txt, C.c_void_p).value
        return bytes((C.c_char * nb.value).from_address(addr)) if nb.value else b""

    def sam_text_device(self, contigs, contig_ids) -> bytes:
        """the SAM records of output_mapping (quick_map3.c:152-181) for these contigs, formatted on the device"""
        raw, n, ln = contigs if isinstance(contigs, tuple) else self.pack_strings(contigs)
        enc = [s_.encode() for s_ in contig_ids]
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum([len(e) for e in enc])
        txt, nb = C.c_char_p(), C.c_uint64()
        check(self.L.vdjx_sam_text(self.h, raw, n, ln, b"".join(enc), _p(off), C.byref(txt), C.byref(nb)), "vdjx_sam_text")
        # (C.string_at takes a C int: the text of 10 M pairs is 3 GB)
        addr = C.cast(txt, C.c_void_p).value
        return bytes((C.c_char * nb.value).from_address(addr)) if nb.value else b""

    def _contig_block(self, contigs, who):
        """pack_strings' tuple as it is, or equally long strings packed -> (raw, n, ln)"""
        if isinstance(contigs, tuple):
            return contigs
        if len({len(s_) for s_ in contigs}) > 1:
            raise VdjxError(f"{who}: contigs of unequal length")
        return self.pack_strings(contigs)

    def quant(self, contigs, max_iter: int = 10000, tol: float = 1e-5):
        """vdjx_quant: expected read pairs per contig (RSEM's paired-end EM over map_emit's placements, on the device)
        -> (counts float64[n], info dict: pairs, alignments, unique_pairs, iterations, converged, eff_len)"""
        raw, n, ln = self._contig_block(contigs, "vdjx_quant")
        counts = np.zeros(n, np.float64)
        info = _lib.QuantInfo()
        prm = _lib.QuantParams(int(max_iter), float(tol))
        check(self.L.vdjx_quant(self.h, raw, n, ln, C.byref(prm), _p(counts), C.byref(info)), "vdjx_quant")
        return counts, self._quant_info(info)

    @staticmethod
    def _placements(who, offsets, pairs):
        """the placements of quant_pairs / quant_pairs_boot -> (offsets uint64[n + 1], PAIR_DTYPE array, n)"""
        offs = _c(offsets, np.uint64)
        if offs.ndim != 1 or offs.shape[0] < 1:
            raise VdjxError(f"{who}: offsets must hold n + 1 entries")
        n = offs.shape[0] - 1
        if isinstance(pairs, tuple):
            pid, ins = (np.asarray(x) for x in pairs)
            if pid.shape != ins.shape or pid.ndim != 1:
                raise VdjxError(f"{who}: pair_id and insert of unequal shape")
            packed = np.zeros(pid.shape[0], PAIR_DTYPE)
            packed["pair_id"] = pid
            packed["insert"] = ins
        else:
            packed = _c(pairs, PAIR_DTYPE)
        if n and packed.shape[0] != int(offs[n]):
            raise VdjxError(f"{who}: {packed.shape[0]} placements, offsets[n]={int(offs[n])}")
        return offs, packed, n

    def quant_pairs(self, offsets, pairs, length: int, n_pairs: int, max_iter: int = 10000, tol: float = 1e-5):
        """vdjx_quant_pairs: the same model over placements the caller brings, in map_emit's shape (contig-major): offsets[n + 1],
        `pairs` a PAIR_DTYPE array of offsets[n] placements or a (pair_id, insert) tuple of arrays, packed here.  Only pair_id and
        insert are read; no pool and no read index are needed.  -> what quant returns"""
        offs, packed, n = self._placements("vdjx_quant_pairs", offsets, pairs)
        counts = np.zeros(n, np.float64)
        info = _lib.QuantInfo()
        prm = _lib.QuantParams(int(max_iter), float(tol))
        check(self.L.vdjx_quant_pairs(self.h, _p(offs), _p(packed), n, int(length), int(n_pairs), C.byref(prm), _p(counts), C.byref(info)),
              "vdjx_quant_pairs")
        return counts, self._quant_info(info)

    @staticmethod
    def _quant_info(info):
        return dict(pairs=int(info.pairs), alignments=int(info.alignments), unique_pairs=int(info.unique_pairs),
                    iterations=int(info.iterations), converged=bool(info.converged), eff_len=float(info.eff_len))

    @staticmethod
    def _quant_boot_result(counts, info, boot, iters, binfo):
        from . import annot
        out = dict(counts=counts, boot=boot, iterations=iters, info=Context._quant_info(info),
                   boot_info=dict(replicates=int(binfo.replicates), converged=int(binfo.converged), batches=int(binfo.batches),
                                  max_iterations=int(binfo.max_iterations), iterations=int(binfo.iterations)))
        out.update(annot.quant_boot_summary(boot))
        return out

    def quant_boot(self, contigs, replicates: int = 100, seed: int = 1, max_iter: int = 10000, tol: float = 1e-5):
        """vdjx_quant_boot: quant's point estimate and `replicates` bootstrap replicates of it over the placed pairs -> dict: counts
        float64[n] and info (quant's), boot float64[B, n], mean / sd / lower / upper float64[n] (vdjx_quant_boot_summary), iterations
        uint32[B], boot_info (replicates, converged, batches, max_iterations, iterations)"""
        raw, n, ln = self._contig_block(contigs, "vdjx_quant_boot")
        b = int(replicates)
        rows = b if 1 <= b <= 1024 else 1
        counts, boot, iters = np.zeros(n, np.float64), np.zeros((rows, n), np.float64), np.zeros(rows, np.uint32)
        info, binfo = _lib.QuantInfo(), _lib.QuantBootInfo()
        prm, bprm = _lib.QuantParams(int(max_iter), float(tol)), _lib.QuantBootParams(b, int(seed))
        check(self.L.vdjx_quant_boot(self.h, raw, n, ln, C.byref(prm), C.byref(bprm), _p(counts), C.byref(info), _p(boot), _p(iters),
                                     C.byref(binfo)), "vdjx_quant_boot")
        return self._quant_boot_result(counts, info, boot, iters, binfo)

    def quant_pairs_boot(self, offsets, pairs, length: int, n_pairs: int, replicates: int = 100, seed: int = 1, mult=None,
                         return_mult: bool = False, max_iter: int = 10000, tol: float = 1e-5):
        """vdjx_quant_pairs_boot: quant_boot over placements the caller brings (quant_pairs' arguments).  mult: None, or uint32[B, n_pairs]
        multiplicities by replicate and pair id that replace the draws (a weighted EM); return_mult: also "mult", the multiplicities
        used (0 for ids without a placement).  -> what quant_boot returns"""
        offs, packed, n = self._placements("vdjx_quant_pairs_boot", offsets, pairs)
        b = int(replicates)
        rows = b if 1 <= b <= 1024 else 1
        m_in = m_out = None
        if mult is not None:
            m_in = _c(mult, np.uint32)
            if m_in.shape != (rows, int(n_pairs)):
                raise VdjxError(f"vdjx_quant_pairs_boot: mult of shape {m_in.shape}, not ({rows}, {int(n_pairs)})")
        if return_mult:
            m_out = np.zeros((rows, int(n_pairs)), np.uint32)
        counts, boot, iters = np.zeros(n, np.float64), np.zeros((rows, n), np.float64), np.zeros(rows, np.uint32)
        info, binfo = _lib.QuantInfo(), _lib.QuantBootInfo()
        prm, bprm = _lib.QuantParams(int(max_iter), float(tol)), _lib.QuantBootParams(b, int(seed))
        check(self.L.vdjx_quant_pairs_boot(self.h, _p(offs), _p(packed), n, int(length), int(n_pairs), C.byref(prm), C.byref(bprm),
                                           _p(m_in) if m_in is not None else None, _p(m_out) if m_out is not None else None, _p(counts),
                                           C.byref(info), _p(boot), _p(iters), C.byref(binfo)), "vdjx_quant_pairs_boot")
        out = self._quant_boot_result(counts, info, boot, iters, binfo)
        if return_mult:
            out["mult"] = m_out
        return out

    def germline_load(self, names_or_records):
        """vdjx_germline_load: a germline FASTA (path) or a list of (FASTA header, sequence) records -> dict(names, classes, skipped).
        Names, classes and sequences as include/vdjx.h states (vdjer_amd/annot.py); the set stays on the device."""
        from . import annot
        recs = annot.read_fasta(names_or_records) if isinstance(names_or_records, str) else list(names_or_records)
        parsed = [annot.parse_record(h, q) for h, q in recs]
        names = [x[0] for x in parsed]
        cls = "".join(x[1] if x[1] in "VJ" else "-" for x in parsed)
        seqs = [x[2] for x in parsed]
        off = np.zeros(len(seqs) + 1, np.uint64)
        off[1:] = np.cumsum([len(q) for q in seqs], dtype=np.uint64)
        check(self.L.vdjx_germline_load(self.h, "".join(seqs).encode(), _p(off), cls.encode(), len(seqs)), "vdjx_germline_load")
        skipped = {}
        for x in parsed:
            if x[1] not in "VJ":
                skipped[x[1]] = skipped.get(x[1], 0) + 1
        self._germ_names = names
        return dict(names=names, classes=[x[1] for x in parsed], skipped=skipped)

    ANNOT_HIT = np.dtype([("gene", "<i4"), ("score", "<i4"), ("n_tied", "<i4"), ("tied", "<i4", (8,)), ("seq_start", "<i4"),
                          ("seq_end", "<i4"), ("germ_start", "<i4"), ("germ_end", "<i4"), ("matches", "<i4"), ("mismatches", "<i4"),
                          ("ins", "<i4"), ("del", "<i4"), ("opens", "<i4"), ("n_runs", "<i4"), ("runs", "<u4", (64,))])

    def annotate(self, contigs, match: int = 2, mismatch: int = 3, gap_open: int = 5, gap_extend: int = 2, min_v_score: int = 40,
                 min_j_score: int = 20):
        """vdjx_annotate: V and J hits of every contig against the loaded germlines -> {"v": {field: array}, "j": {...}}, the fields of
        vdjx_annot_hit (tied: [n, 8], runs: [n, 64])"""
        raw, n, ln = self._contig_block(contigs, "vdjx_annotate")
        hv = np.zeros(n, self.ANNOT_HIT)
        hj = np.zeros(n, self.ANNOT_HIT)
        prm = _lib.AnnotParams(int(match), int(mismatch), int(gap_open), int(gap_extend), int(min_v_score), int(min_j_score))
        check(self.L.vdjx_annotate(self.h, raw, n, ln, C.byref(prm), _p(hv), _p(hj)), "vdjx_annotate")
        return {k: {f: h[f].copy() for f in self.ANNOT_HIT.names} for k, h in (("v", hv), ("j", hj))}

    def constant_load(self, fasta_path_or_records):
        """vdjx_constant_load: a constant-region FASTA (path) or a list of (FASTA header, sequence) records -> dict(names).  Names and
        sequences as for germline_load (vdjer_amd/annot.py); every record is a constant record.  The set stays on the device, beside the
        germline set."""
        from . import annot
        recs = annot.read_fasta(fasta_path_or_records) if isinstance(fasta_path_or_records, str) else list(fasta_path_or_records)
        names = [annot.parse_name(h) for h, _ in recs]
        seqs = [annot.clean_seq(q) for _, q in recs]
        off = np.zeros(len(seqs) + 1, np.uint64)
        off[1:] = np.cumsum([len(q) for q in seqs], dtype=np.uint64)
        check(self.L.vdjx_constant_load(self.h, "".join(seqs).encode(), _p(off), len(seqs)), "vdjx_constant_load")
        self._const_n = len(seqs)
        return dict(names=names)

    def isotype(self, contigs, tail: int = 48, match: int = 2, mismatch: int = 3, gap_open: int = 5, gap_extend: int = 2,
                min_score: int = 48, scores: bool = True):
        """vdjx_isotype: the last `tail` bases of every contig against the loaded constant set -> {"c": {field: array}, "scores":
        int32[n, C] | None}, the fields of vdjx_annot_hit (seq_start / seq_end in contig coordinates)"""
        raw, n, ln = self._contig_block(contigs, "vdjx_isotype")
        hc = np.zeros(n, self.ANNOT_HIT)
        nc = getattr(self, "_const_n", 0)
        sc = np.zeros((n, nc), np.int32) if scores else None
        prm = _lib.IsotypeParams(int(match), int(mismatch), int(gap_open), int(gap_extend), int(min_score), int(tail))
        check(self.L.vdjx_isotype(self.h, raw, n, ln, C.byref(prm), _p(hc), _p(sc) if scores and sc.size else None), "vdjx_isotype")
        return {"c": {f: hc[f].copy() for f in self.ANNOT_HIT.names}, "scores": sc}

    def dsegment_load(self, fasta_path_or_records):
        """vdjx_dsegment_load: a germline FASTA (path) or a list of (FASTA header, sequence) records -> dict(names, skipped).  The records
        whose class (vdjer_amd/annot.py parse_class) is D are kept and loaded, the others counted per class in `skipped`.  The set stays
        on the device, beside the germline and the constant set."""
        from . import annot
        recs = annot.read_fasta(fasta_path_or_records) if isinstance(fasta_path_or_records, str) else list(fasta_path_or_records)
        parsed = [annot.parse_record(h, q) for h, q in recs]
        kept = [x for x in parsed if x[1] == "D"]
        skipped = {}
        for x in parsed:
            if x[1] != "D":
                skipped[x[1]] = skipped.get(x[1], 0) + 1
        seqs = [x[2] for x in kept]
        off = np.zeros(len(seqs) + 1, np.uint64)
        off[1:] = np.cumsum([len(q) for q in seqs], dtype=np.uint64)
        check(self.L.vdjx_dsegment_load(self.h, "".join(seqs).encode(), _p(off), len(seqs)), "vdjx_dsegment_load")
        self._dseg_n = len(seqs)
        return dict(names=[x[0] for x in kept], skipped=skipped)

    def dcall(self, contigs, win_start, win_len, match: int = 2, mismatch: int = 3, gap_open: int = 5, gap_extend: int = 2,
              min_score: int = 22, scores: bool = True):
        """vdjx_dcall: contig c's window [win_start[c], win_start[c] + win_len[c]) (0-based, at most 256 bases) against the loaded D set
        -> {"d": {field: array}, "scores": int32[n, C] | None}, the fields of vdjx_annot_hit (seq_start / seq_end in contig coordinates)"""
        raw, n, ln = self._contig_block(contigs, "vdjx_dcall")
        ws = np.ascontiguousarray(win_start, np.int32)
        wl = np.ascontiguousarray(win_len, np.int32)
        if ws.shape != (n,) or wl.shape != (n,):
            raise VdjxError(f"vdjx_dcall: {n} contigs, win_start of shape {ws.shape}, win_len of shape {wl.shape}")
        hd = np.zeros(n, self.ANNOT_HIT)
        nc = getattr(self, "_dseg_n", 0)
        sc = np.zeros((n, nc), np.int32) if scores else None
        prm = _lib.DcallParams(int(match), int(mismatch), int(gap_open), int(gap_extend), int(min_score))
        check(self.L.vdjx_dcall(self.h, raw, n, ln, _p(ws), _p(wl), C.byref(prm), _p(hd), _p(sc) if scores and sc.size else None), "vdjx_dcall")
        return {"d": {f: hd[f].copy() for f in self.ANNOT_HIT.names}, "scores": sc}

    MUT_ROW = np.dtype([(f, "<i4") for f in ("cols", "v_r", "v_s", "v_stop", "v_na", "v_codons", "j_mis", "flags")])
    MUT_INFO_FIELDS = ("contigs", "aligned", "cols", "v_r", "v_s", "v_stop", "v_na", "v_codons", "truncated", "clipped")

    def _hit_array(self, h, n, what, who):
        """the field dict of annotate() / dcall() as an array of vdjx_annot_hit; who: the call's name in the message"""
        out = np.zeros(n, self.ANNOT_HIT)
        for f in self.ANNOT_HIT.names:
            a = np.asarray(h[f])
            if a.shape != out[f].shape:
                raise VdjxError(f"{who}: {n} contigs, {what}[{f!r}] of shape {a.shape}")
            out[f] = a
        return out

    def mutations(self, contigs, v, j, d=None, limit=None, rows: bool = True):
        """vdjx_mutations: every contig and its V(D)J germline side by side, and the V segment's replacement / silent / stop mutation
        counts.  v, j, d: the field dicts annotate() and dcall() return (d may be None); limit: int32[n] or None (the contig's length)
        -> {"seq", "germ", "mask": list[str] | None (rows=False: no row is fetched), "counts": {field: int32[n]} (cols, v_r, v_s, v_stop,
        v_na, v_codons, j_mis, flags), "info": dict}"""
        raw, n, ln = self._contig_block(contigs, "vdjx_mutations")
        hv, hj = self._hit_array(v, n, "v", "vdjx_mutations"), self._hit_array(j, n, "j", "vdjx_mutations")
        hd = None if d is None else self._hit_array(d, n, "d", "vdjx_mutations")
        lim = None if limit is None else np.ascontiguousarray(limit, np.int32)
        if lim is not None and lim.shape != (n,):
            raise VdjxError(f"vdjx_mutations: {n} contigs, limit of shape {lim.shape}")
        off = np.zeros(n + 1, np.uint64)
        check(self.L.vdjx_mutations_layout(_p(hv), _p(hd), _p(hj), n, _p(off)), "vdjx_mutations_layout")
        total = int(off[n])
        bufs = [np.zeros(max(total, 1), np.uint8) for _ in range(3)] if rows else [None] * 3
        out = np.zeros(n, self.MUT_ROW)
        info = _lib.MutInfo()
        check(self.L.vdjx_mutations(self.h, raw, n, ln, _p(hv), _p(hd), _p(hj), _p(lim), _p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(out),
                                    C.byref(info)), "vdjx_mutations")
        text = [None] * 3
        if rows:
            for k in range(3):
                b = bufs[k].tobytes()
                text[k] = [b[int(off[i]):int(off[i + 1])].decode("latin-1") for i in range(n)]
        return {"seq": text[0], "germ": text[1], "mask": text[2], "counts": {f: out[f].copy() for f in self.MUT_ROW.names},
                "info": {f: int(getattr(info, f)) for f in self.MUT_INFO_FIELDS}}

    SEL_COUNTS = np.dtype([("obs_r", "<i4", 2), ("obs_s", "<i4", 2), ("codons", "<i4", 2), ("flags", "<u4"), ("pad", "<u4"), ("exp_r", "<u8", 2),
                           ("exp_s", "<u8", 2)])
    SEL_STAT = np.dtype([("sequences", "<u4"), ("pad", "<u4"), ("x", "<u8"), ("n", "<u8"), ("exp_r", "<u8"), ("exp_s", "<u8"), ("sigma", "<f8"),
                         ("lower", "<f8"), ("upper", "<f8"), ("p_positive", "<f8")])
    SEL_INFO_FIELDS = ("contigs", "used", "no_regions", "truncated", "groups", "regions", "chunks", "large_rows")

    def selection(self, contigs, v, limit=None, cdr=None, weight=None, group=None, groups=None, pdf: bool = False):
        """vdjx_selection: the observed R / S counts of the V segment per region, the expected R / S weights of its germline codons and the
        posterior of the selection strength per contig, per group and for all contigs.  v: the field dict annotate() returns; limit:
        int32[n] or None; cdr: int32[records, 4] (annot.read_v_regions) or None (one region); weight: uint32[1024, 4]
        (annot.read_targeting) or None (uniform); group: int32[n] (negative: in no group) or None; groups: G (None: max(group) + 1)
        -> {"counts": {field: array[n] or [n, 2]}, "stat": {field: array[n + G + 1, K]}, "pdf": float64[G + 1, K, 4001] | None, "info":
        dict}"""
        raw, n, ln = self._contig_block(contigs, "vdjx_selection")
        hv = self._hit_array(v, n, "v", "vdjx_selection")
        lim = None if limit is None else np.ascontiguousarray(limit, np.int32)
        if lim is not None and lim.shape != (n,):
            raise VdjxError(f"vdjx_selection: {n} contigs, limit of shape {lim.shape}")
        reg = None if cdr is None else np.ascontiguousarray(cdr, np.int32)
        if reg is not None and (reg.ndim != 2 or reg.shape[1] != 4):
            raise VdjxError(f"vdjx_selection: cdr of shape {reg.shape}")
        w = None if weight is None else np.ascontiguousarray(weight, np.uint32)
        if w is not None and w.shape != (1024, 4):
            raise VdjxError(f"vdjx_selection: weight of shape {w.shape}")
        grp = None if group is None else np.ascontiguousarray(group, np.int32)
        if grp is not None and grp.shape != (n,):
            raise VdjxError(f"vdjx_selection: {n} contigs, group of shape {grp.shape}")
        g = int(groups) if groups is not None else (int(grp.max()) + 1 if grp is not None and n and int(grp.max()) >= 0 else 0)
        if not 0 <= g < 1 << 32:
            raise VdjxError(f"vdjx_selection: {g} groups")
        k = 1 if reg is None else 2
        big = g >= 1 << 20                                            # (a count the library refuses: nothing is written)
        counts = np.zeros(n, self.SEL_COUNTS)
        stat = np.zeros((1 if big else n + g + 1, k), self.SEL_STAT)
        dens = (np.zeros((g + 1, k, 4001)) if g + 1 <= 65536 else np.zeros(1)) if pdf else None      # (as above: refused, not written)
        info = _lib.SelInfo()
        check(self.L.vdjx_selection(self.h, raw, n, ln, _p(hv), _p(lim), _p(reg), 0 if reg is None else reg.shape[0], _p(w), _p(grp), g,
                                    _p(counts), _p(stat), _p(dens), C.byref(info)), "vdjx_selection")
        return {"counts": {f: counts[f].copy() for f in self.SEL_COUNTS.names if f != "pad"},
                "stat": {f: stat[f].copy() for f in self.SEL_STAT.names if f != "pad"}, "pdf": dens,
                "info": {f: int(getattr(info, f)) for f in self.SEL_INFO_FIELDS}}

    SELCONV_INFO_FIELDS = ("members", "leaves", "combines", "groups", "regions", "rows", "levels", "batches")

    def selection_convolve(self, counts, regions, group=None, groups=None, pdf: bool = False):
        """vdjx_selection_convolve: BASELINe's group posteriors -- per group and for all contigs the distribution of the mean of the
        contributing members' independent sigmas (their own posteriors, convolved).  counts: the "counts" dict selection() returns (or
        handmade: obs_r, obs_s, exp_r, exp_s of shape [n, 2]; codons and flags are not read); regions: K, 1 or 2; group: int32[n]
        (negative: in no group) or None; groups: G (None: max(group) + 1) -> {"stat": {field: array[G + 1, K]}, "pdf": float64[G + 1, K,
        4001] | None, "info": dict}"""
        n = len(np.asarray(counts["obs_r"]))
        raw = np.zeros(n, self.SEL_COUNTS)
        for f in ("obs_r", "obs_s", "exp_r", "exp_s"):
            a = np.asarray(counts[f])
            if a.shape != (n, 2):
                raise VdjxError(f"vdjx_selection_convolve: {n} contigs, {f} of shape {a.shape}")
            raw[f] = a
        for f in ("codons", "flags"):
            if f in counts:
                raw[f] = np.asarray(counts[f])
        grp = None if group is None else np.ascontiguousarray(group, np.int32)
        if grp is not None and grp.shape != (n,):
            raise VdjxError(f"vdjx_selection_convolve: {n} contigs, group of shape {grp.shape}")
        g = int(groups) if groups is not None else (int(grp.max()) + 1 if grp is not None and n and int(grp.max()) >= 0 else 0)
        k = int(regions)
        if not 0 <= g < 1 << 32 or not 0 <= k < 1 << 32:
            raise VdjxError(f"vdjx_selection_convolve: {g} groups, {k} regions")
        refused = g >= 1 << 20 or not 1 <= k <= 2                       # (what the library refuses: nothing is written)
        stat = np.zeros((1, 1) if refused else (g + 1, k), self.SEL_STAT)
        dens = (np.zeros(1) if refused or g + 1 > 65536 else np.zeros((g + 1, k, 4001))) if pdf else None
        info = _lib.SelConvInfo()
        check(self.L.vdjx_selection_convolve(self.h, _p(raw), n, k, _p(grp), g, _p(stat), _p(dens), C.byref(info)), "vdjx_selection_convolve")
        return {"stat": {f: stat[f].copy() for f in self.SEL_STAT.names if f != "pad"}, "pdf": dens,
                "info": {f: int(getattr(info, f)) for f in self.SELCONV_INFO_FIELDS}}

    TGT_INFO_FIELDS = ("contigs", "used", "truncated", "units", "positions", "obs_s", "obs_r", "opp_s", "opp_r", "batches")

    def targeting_counts(self, contigs, v, limit=None, group=None):
        """vdjx_targeting_counts: per 5-mer and new base the observed changes and the opportunities of the V segments, silent and
        replacement apart, a (group, V record) pair counted once.  v: the field dict annotate() returns; limit: int32[n] or None; group:
        int32[n] (negative: in no group) or None -> {"counts": uint64[2, 2, 1024, 4] (kind: observed, opportunity; class: silent,
        replacement; 5-mer; new base), "info": dict}.  annot.targeting_model makes the weights of them."""
        raw, n, ln = self._contig_block(contigs, "vdjx_targeting_counts")
        hv = self._hit_array(v, n, "v", "vdjx_targeting_counts")
        lim = None if limit is None else np.ascontiguousarray(limit, np.int32)
        if lim is not None and lim.shape != (n,):
            raise VdjxError(f"vdjx_targeting_counts: {n} contigs, limit of shape {lim.shape}")
        grp = None if group is None else np.ascontiguousarray(group, np.int32)
        if grp is not None and grp.shape != (n,):
            raise VdjxError(f"vdjx_targeting_counts: {n} contigs, group of shape {grp.shape}")
        counts = np.zeros((2, 2, 1024, 4), np.uint64)
        info = _lib.TgtInfo()
        check(self.L.vdjx_targeting_counts(self.h, raw, n, ln, _p(hv), _p(lim), _p(grp), _p(counts), C.byref(info)), "vdjx_targeting_counts")
        return {"counts": counts, "info": {f: int(getattr(info, f)) for f in self.TGT_INFO_FIELDS}}

    CONS_UNIT = np.dtype([("group", "<i4"), ("gene", "<i4"), ("members", "<u4"), ("off_record", "<u4"), ("lo", "<i4"), ("hi", "<i4"), ("off", "<u8")])
    CONS_INFO_FIELDS = ("contigs", "used", "truncated", "off_record", "units", "columns", "votes", "inserted", "undecided", "batches",
                        "large_units")

    def consensus(self, contigs, v, limit=None, group=None, min_freq=(6000, 10000), counts: bool = False):
        """vdjx_consensus: per unit (a group, or a contig on its own) the sequence its voters agree on, column by column over the unit's V
        record, and the record's own bases beside it.  v: the field dict annotate() returns; limit: int32[n] or None; group: int32[n]
        (negative: in no group) or None; min_freq: (num, den), a column's winner needs best * den >= num * cover ((0, 1): the most
        common symbol) -> {"unit": int32[n] (the voter's unit, -1: none), "units": {field: array[U]} (group, gene, members, off_record, lo,
        hi, off), "cons", "germ": list[str] per unit (cons over ACGTN-), "cover", "best": list of uint32 arrays per unit | None
        (counts=False), "info": dict}.  annot.consensus_hits makes contigs and V hits of the rows."""
        raw, n, ln = self._contig_block(contigs, "vdjx_consensus")
        hv = self._hit_array(v, n, "v", "vdjx_consensus")
        lim = None if limit is None else np.ascontiguousarray(limit, np.int32)
        if lim is not None and lim.shape != (n,):
            raise VdjxError(f"vdjx_consensus: {n} contigs, limit of shape {lim.shape}")
        grp = None if group is None else np.ascontiguousarray(group, np.int32)
        if grp is not None and grp.shape != (n,):
            raise VdjxError(f"vdjx_consensus: {n} contigs, group of shape {grp.shape}")
        unit = np.full(n, -1, np.int32)
        units = np.zeros(max(n, 1), self.CONS_UNIT)
        nu, ncol = C.c_uint64(0), C.c_uint64(0)
        info = _lib.ConsInfo()
        prm = _lib.ConsParams(int(min_freq[0]), int(min_freq[1]))
        # the sizes first; whatever the layout refuses the call refuses under its own name (with nothing to write into)
        total = 0
        if self.L.vdjx_consensus_layout(_p(hv), _p(lim), _p(grp), n, ln, _p(unit), _p(units), C.byref(nu), C.byref(ncol)) == 0:
            total = int(ncol.value)
        rows = [np.zeros(max(total, 1), np.uint8) for _ in range(2)]
        cnt = [np.zeros(max(total, 1), np.uint32) for _ in range(2)] if counts else [None, None]
        check(self.L.vdjx_consensus(self.h, raw, n, ln, _p(hv), _p(lim), _p(grp), C.byref(prm), _p(rows[0]), _p(rows[1]), _p(cnt[0]), _p(cnt[1]),
                                    _p(units), _p(unit), C.byref(info)), "vdjx_consensus")
        U = int(info.units)
        units = units[:U]
        cut = [(int(o), int(o) + int(h) - int(l)) for o, l, h in zip(units["off"], units["lo"], units["hi"])]
        text = [r.tobytes() for r in rows]
        return {"unit": unit, "units": {f: units[f].copy() for f in self.CONS_UNIT.names},
                "cons": [text[0][a:b].decode("latin-1") for a, b in cut], "germ": [text[1][a:b].decode("latin-1") for a, b in cut],
                "cover": [cnt[0][a:b].copy() for a, b in cut] if counts else None,
                "best": [cnt[1][a:b].copy() for a, b in cut] if counts else None,
                "info": {f: int(getattr(info, f)) for f in self.CONS_INFO_FIELDS}}

    LINEAGE_NONE = 0xFFFFFFFF                                # VDJX_LINEAGE_NONE (include/vdjx.h)

    LINEAGE_SYMMETRY = {"avg": 0, "min": 1}                  # vdjx_lineage_model_params.symmetry

    def lineage(self, junctions, group, max_dist=(1500, 10000), nearest: bool = True, table=None, symmetry="avg"):
        """vdjx_lineage: single linkage inside the buckets of equal group and junction length; two junctions are linked when
        d * max_dist[1] <= max_dist[0] * L (d: positions that differ or are not ACGT).  junctions: str or bytes per item; group: uint32[n],
        LINEAGE_NONE for an item that takes no part -> {"clone": int32[n] (0-based, -1: no part), "nearest": int32[n] | None (smallest
        non-zero distance inside the bucket, -1: none), "info": dict(items, buckets, largest_bucket, clones, pairs, links)}.
        table: uint16[1024, 4] (annot.lineage_distance_table) -> vdjx_lineage_model instead: the 5-mer substitution distance D, linked when
        D * max_dist[1] <= 2000 * max_dist[0] * L, nearest in the same units; symmetry: "avg" (both directions added) or "min" (twice the
        smaller).  Without a table the call is vdjx_lineage's and symmetry is not looked at.  (Complete and average linkage: lineage_link.)"""
        enc = [s_ if isinstance(s_, (bytes, bytearray)) else s_.encode() for s_ in junctions]
        n = len(enc)
        grp = np.ascontiguousarray(group, np.uint32)
        if grp.shape != (n,):
            raise VdjxError(f"vdjx_lineage: {n} junctions, group of shape {grp.shape}")
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum([len(e) for e in enc], dtype=np.uint64)
        clone = np.zeros(n, np.int32)
        near = np.zeros(n, np.int32) if nearest else None
        info = _lib.LineageInfo()
        if table is None:
            prm = _lib.LineageParams(int(max_dist[0]), int(max_dist[1]))
            check(self.L.vdjx_lineage(self.h, b"".join(enc), _p(off), _p(grp), n, C.byref(prm), _p(clone), _p(near), C.byref(info)), "vdjx_lineage")
        else:
            tab = np.ascontiguousarray(table, np.uint16)
            if tab.shape != (1024, 4) or not np.array_equal(tab, np.asarray(table)):
                raise VdjxError(f"vdjx_lineage_model: a table of shape {np.shape(table)}, not uint16[1024, 4]")
            sym = self.LINEAGE_SYMMETRY.get(symmetry, symmetry)
            if not isinstance(sym, (int, np.integer)):
                raise VdjxError(f"vdjx_lineage_model: symmetry {symmetry!r} (avg or min)")
            prm = _lib.LineageModelParams(int(max_dist[0]), int(max_dist[1]), int(sym))
            check(self.L.vdjx_lineage_model(self.h, b"".join(enc), _p(off), _p(grp), n, C.byref(prm), _p(tab), _p(clone), _p(near), C.byref(info)),
                  "vdjx_lineage_model")
        return {"clone": clone, "nearest": near,
                "info": {f: int(getattr(info, f)) for f in ("items", "buckets", "largest_bucket", "clones", "pairs", "links")}}

    LINEAGE_LINKAGE = {"single": 0, "complete": 1, "average": 2}      # vdjx_lineage_link_params.linkage
    LINEAGE_LINK_FIELDS = ("components", "largest_component", "merges", "clones_single", "batches", "cells")

    def lineage_link(self, junctions, group, max_dist=(1500, 10000), nearest: bool = True, table=None, symmetry="avg", link="complete"):
        """vdjx_lineage_link: lineage()'s arguments, buckets, distances (Hamming, or the 5-mer distance of `table`) and nearest, the clusters
        cut at the same threshold under another linkage.  link: "complete" or "average" ("single", or the numbers 0 .. 2: 0 gives lineage()'s
        bits through this entry point) -> lineage()'s result, info["clones"] the final number, and one more key, "link": dict(components,
        largest_component, merges, clones_single, batches, cells) -- all zero under single linkage."""
        enc = [s_ if isinstance(s_, (bytes, bytearray)) else s_.encode() for s_ in junctions]
        n = len(enc)
        grp = np.ascontiguousarray(group, np.uint32)
        if grp.shape != (n,):
            raise VdjxError(f"vdjx_lineage_link: {n} junctions, group of shape {grp.shape}")
        linkage = self.LINEAGE_LINKAGE.get(link, link) if isinstance(link, str) else link
        if not isinstance(linkage, (int, np.integer)):
            raise VdjxError(f"vdjx_lineage_link: link {link!r} (single, complete or average)")
        tab = None
        if table is not None:
            tab = np.ascontiguousarray(table, np.uint16)
            if tab.shape != (1024, 4) or not np.array_equal(tab, np.asarray(table)):
                raise VdjxError(f"vdjx_lineage_link: a table of shape {np.shape(table)}, not uint16[1024, 4]")
        sym = self.LINEAGE_SYMMETRY.get(symmetry, symmetry)
        if not isinstance(sym, (int, np.integer)):
            raise VdjxError(f"vdjx_lineage_link: symmetry {symmetry!r} (avg or min)")
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum([len(e) for e in enc], dtype=np.uint64)
        clone = np.zeros(n, np.int32)
        near = np.zeros(n, np.int32) if nearest else None
        info, linfo = _lib.LineageInfo(), _lib.LineageLinkInfo()
        prm = _lib.LineageLinkParams(int(max_dist[0]), int(max_dist[1]), int(sym), int(linkage))
        check(self.L.vdjx_lineage_link(self.h, b"".join(enc), _p(off), _p(grp), n, C.byref(prm), _p(tab), _p(clone), _p(near), C.byref(info),
                                       C.byref(linfo)), "vdjx_lineage_link")
        return {"clone": clone, "nearest": near,
                "info": {f: int(getattr(info, f)) for f in ("items", "buckets", "largest_bucket", "clones", "pairs", "links")},
                "link": {f: int(getattr(linfo, f)) for f in self.LINEAGE_LINK_FIELDS}}

    THRESHOLD_STATUS = _lib.THRESHOLD_STATUS                 # info["status"] by name (VDJX_THRESHOLD_FOUND .. _SHALLOW)
    THRESHOLD_FIELDS = ("values", "distinct", "status", "k", "peaks_all", "peaks", "p1_first", "p1_last", "p2_first", "p2_last", "t_first", "t_last",
                        "threshold", "y1", "y2", "m", "ymax")

    def lineage_threshold(self, nearest, length, unit=1, max_k=200, peak_shift=5, valley=(1, 2), min_values=10):
        """vdjx_lineage_threshold: the valley between the two modes of the nearest-neighbour distances.  nearest: int32[n], lineage()'s
        "nearest" (-1: none); length: uint32[n], the junctions' lengths; unit: 1 for Hamming distances, 2000 under a table -> {"hist":
        uint32[10001] (items per bin of 0.0001), "density": uint64[10001] (the smoothed counts at the chosen bandwidth k / 1000, scale 2^30),
        "peaks": uint32[max_k, 2] (all and counted peaks of every bandwidth), "info": dict(values, distinct, status, k, peaks_all, peaks,
        p1_first, p1_last, p2_first, p2_last, t_first, t_last, threshold, y1, y2, m, ymax)}.  info["status"] indexes THRESHOLD_STATUS;
        info["threshold"] is in ten-thousandths, lineage()'s max_dist[0] over 10000, and 0 unless the status is 0."""
        near = np.ascontiguousarray(nearest, np.int32)
        ln = np.ascontiguousarray(length, np.uint32)
        if near.ndim != 1 or ln.shape != near.shape or not np.array_equal(near, np.asarray(nearest)) or not np.array_equal(ln, np.asarray(length)):
            raise VdjxError(f"vdjx_lineage_threshold: nearest int32[n] and length uint32[n], not shapes {np.shape(nearest)} and {np.shape(length)}")
        ints = (unit, max_k, peak_shift, valley[0], valley[1], min_values)
        if not all(isinstance(x, (int, np.integer)) and -(1 << 31) <= int(x) < 1 << 31 for x in ints) or int(unit) < 0:
            raise VdjxError(f"vdjx_lineage_threshold: unit {unit}, max_k {max_k}, peak_shift {peak_shift}, valley {valley}, min_values {min_values}")
        prm = _lib.ThresholdParams(int(max_k), int(peak_shift), int(valley[0]), int(valley[1]), int(min_values))
        rows = int(max_k) if 1 <= int(max_k) <= _lib.THRESHOLD_MAX_K else 1          # (a count the library refuses: nothing is written)
        hist = np.zeros(_lib.THRESHOLD_GRID + 1, np.uint32)
        dens = np.zeros(_lib.THRESHOLD_GRID + 1, np.uint64)
        peaks = np.zeros((rows, 2), np.uint32)
        info = _lib.ThresholdInfo()
        check(self.L.vdjx_lineage_threshold(self.h, _p(near), _p(ln), near.shape[0], int(unit), C.byref(prm), _p(hist), _p(dens), _p(peaks), C.byref(info)),
              "vdjx_lineage_threshold")
        return {"hist": hist, "density": dens, "peaks": peaks, "info": {f: int(getattr(info, f)) for f in self.THRESHOLD_FIELDS}}

    TREE_FIELDS = ("members", "clones", "largest_clone", "rounds", "edges", "weight")

    def tree(self, contigs, clone, anchor, prio=None):
        """vdjx_tree: the minimum spanning tree of every clone under the Hamming distance over the members' common window around their
        anchors, rooted at the member of smallest (prio, index).  contigs: equally long strings (or pack_strings' tuple); clone: int32[n],
        -1 for an item that takes no part; anchor: int32[n], 0 .. len; prio: uint32[n] or None -> {"parent", "dist", "depth": int32[n]
        (-1: no part; parent and dist -1 for a root), "info": dict(members, clones, largest_clone, rounds, edges, weight)}"""
        raw, n, ln = self._contig_block(contigs, "vdjx_tree")
        cl = np.ascontiguousarray(clone, np.int32)
        an = np.ascontiguousarray(anchor, np.int32)
        pr = None if prio is None else np.ascontiguousarray(prio, np.uint32)
        if cl.shape != (n,) or an.shape != (n,) or (pr is not None and pr.shape != (n,)):
            raise VdjxError(f"vdjx_tree: {n} contigs, clone of shape {cl.shape}, anchor of shape {an.shape}")
        parent, dist, depth = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        info = _lib.TreeInfo()
        check(self.L.vdjx_tree(self.h, raw, n, ln, _p(cl), _p(an), _p(pr), _p(parent), _p(dist), _p(depth), C.byref(info)), "vdjx_tree")
        return {"parent": parent, "dist": dist, "depth": depth, "info": {f: int(getattr(info, f)) for f in self.TREE_FIELDS}}

    TREE_SUPPORT_FIELDS = ("members", "clones", "largest_clone", "replicates", "batches", "rounds", "edges", "matched", "full")

    def tree_support(self, contigs, clone, anchor, parent, replicates=100, seed=1):
        """vdjx_tree_support: the delete-half jackknife over the window's columns.  contigs, clone, anchor as tree() takes them; parent:
        int32[n], for every member the item whose edge to it is scored, or -1 (typically tree()'s "parent"); replicates: 1 .. 1024; seed:
        any uint64 -> {"support": int32[n] (the replicates whose tree has the edge {i, parent[i]}; -1 where parent is), "info":
        dict(members, clones, largest_clone, replicates, batches, rounds, edges, matched, full)}"""
        raw, n, ln = self._contig_block(contigs, "vdjx_tree_support")
        cl = np.ascontiguousarray(clone, np.int32)
        an = np.ascontiguousarray(anchor, np.int32)
        pa = np.ascontiguousarray(parent, np.int32)
        if cl.shape != (n,) or an.shape != (n,) or pa.shape != (n,):
            raise VdjxError(f"vdjx_tree_support: {n} contigs, clone of shape {cl.shape}, anchor of shape {an.shape}, parent of shape {pa.shape}")
        if not 0 <= int(replicates) < 1 << 32 or not 0 <= int(seed) < 1 << 64:
            raise VdjxError(f"vdjx_tree_support: replicates {replicates}, seed {seed}")
        params = _lib.TreeSupportParams(int(replicates), int(seed))
        support = np.zeros(n, np.int32)
        info = _lib.TreeSupportInfo()
        check(self.L.vdjx_tree_support(self.h, raw, n, ln, _p(cl), _p(an), _p(pa), C.byref(params), _p(support), C.byref(info)), "vdjx_tree_support")
        return {"support": support, "info": {f: int(getattr(info, f)) for f in self.TREE_SUPPORT_FIELDS}}

    TREE_NJ_FIELDS = ("members", "clones", "largest_clone", "internal", "batches", "negative", "edges", "joins", "cells", "parsimony", "length")

    def tree_nj(self, contigs, clone, anchor, prio=None, ancestors=True):
        """vdjx_tree_nj: the neighbour-joining tree of every clone in 16.16 fixed point over the members' common window, rooted at the member
        of smallest (prio, index), with the inferred nodes' sequences and every edge's mutations by Fitch parsimony.  contigs, clone, anchor,
        prio as tree() takes them -> {"parent" int32, "length" int64 (1/65536), "mutations", "depth", "clone" int32: [nodes] each -- slots
        0 .. n - 1 the items, the inferred nodes from n on, lineage after lineage in ascending clone key (-1: no part; a root has parent -1,
        length 0, mutations -1), "anc": the inferred nodes' windows as str (None with ancestors=False), "info": dict(TREE_NJ_FIELDS)}"""
        raw, n, ln = self._contig_block(contigs, "vdjx_tree_nj")
        cl = np.ascontiguousarray(clone, np.int32)
        an = np.ascontiguousarray(anchor, np.int32)
        pr = None if prio is None else np.ascontiguousarray(prio, np.uint32)
        if cl.shape != (n,) or an.shape != (n,) or (pr is not None and pr.shape != (n,)):
            raise VdjxError(f"vdjx_tree_nj: {n} contigs, clone of shape {cl.shape}, anchor of shape {an.shape}")
        total = C.c_uint64(0)
        check(self.L.vdjx_tree_nj_nodes(_p(cl), n, C.byref(total)), "vdjx_tree_nj_nodes")
        nodes = int(total.value)
        parent, mutations, depth, out_clone = (np.zeros(nodes, np.int32) for _ in range(4))
        length = np.zeros(nodes, np.int64)
        anc = np.zeros((nodes - n, max(ln, 1)), np.uint8) if ancestors else None
        info = _lib.TreeNjInfo()
        check(self.L.vdjx_tree_nj(self.h, raw, n, ln, _p(cl), _p(an), _p(pr), _p(parent), _p(length), _p(mutations), _p(depth), _p(out_clone),
                                  _p(anc), C.byref(info)), "vdjx_tree_nj")
        return {"parent": parent, "length": length, "mutations": mutations, "depth": depth, "clone": out_clone,
                "anc": None if anc is None else [row.tobytes().split(b"\0", 1)[0].decode("latin-1") for row in anc],
                "info": {f: int(getattr(info, f)) for f in self.TREE_NJ_FIELDS}}

    TREE_MP_FIELDS = ("members", "clones", "largest_clone", "internal", "batches", "searched", "moved", "rounds", "edges", "moves", "candidates",
                      "parsimony_start", "parsimony")

    def tree_mp(self, contigs, clone, anchor, prio=None, start=None, max_rounds=0, ancestors=True, _reserved=0):
        """vdjx_tree_mp: inside every clone, a search over nearest-neighbour interchanges for the tree of fewest Fitch mutations, from
        tree_nj's tree (start=None) or from the caller's (start: int32[nodes], parents in tree_nj's slots); max_rounds caps a lineage's
        scoring rounds (0: until no interchange lowers the total).  contigs, clone, anchor, prio as tree_nj() takes them -> {"parent",
        "mutations", "depth", "clone" int32: [nodes] each, in tree_nj's slots (a root has parent -1 and mutations -1), "anc": the inferred
        nodes' windows as str (None with ancestors=False), "info": dict(TREE_MP_FIELDS)}.  An edge's length is its mutations."""
        raw, n, ln = self._contig_block(contigs, "vdjx_tree_mp")
        cl = np.ascontiguousarray(clone, np.int32)
        an = np.ascontiguousarray(anchor, np.int32)
        pr = None if prio is None else np.ascontiguousarray(prio, np.uint32)
        if cl.shape != (n,) or an.shape != (n,) or (pr is not None and pr.shape != (n,)):
            raise VdjxError(f"vdjx_tree_mp: {n} contigs, clone of shape {cl.shape}, anchor of shape {an.shape}")
        total = C.c_uint64(0)
        check(self.L.vdjx_tree_nj_nodes(_p(cl), n, C.byref(total)), "vdjx_tree_nj_nodes")
        nodes = int(total.value)
        sp = None if start is None else np.ascontiguousarray(start, np.int32)
        if sp is not None and sp.shape != (nodes,):
            raise VdjxError(f"vdjx_tree_mp: start of shape {sp.shape} for {nodes} nodes")
        if not 0 <= int(max_rounds) < 1 << 32:
            raise VdjxError(f"vdjx_tree_mp: max_rounds {max_rounds}")
        params = _lib.TreeMpParams(int(max_rounds), int(_reserved))
        parent, mutations, depth, out_clone = (np.zeros(nodes, np.int32) for _ in range(4))
        anc = np.zeros((nodes - n, max(ln, 1)), np.uint8) if ancestors else None
        info = _lib.TreeMpInfo()
        check(self.L.vdjx_tree_mp(self.h, raw, n, ln, _p(cl), _p(an), _p(pr), _p(sp), C.byref(params), _p(parent), _p(mutations), _p(depth),
                                  _p(out_clone), _p(anc), C.byref(info)), "vdjx_tree_mp")
        return {"parent": parent, "mutations": mutations, "depth": depth, "clone": out_clone,
                "anc": None if anc is None else [row.tobytes().split(b"\0", 1)[0].decode("latin-1") for row in anc],
                "info": {f: int(getattr(info, f)) for f in self.TREE_MP_FIELDS}}

    TREE_SPR_FIELDS = TREE_MP_FIELDS

    def tree_spr(self, contigs, clone, anchor, prio=None, start=None, max_rounds=0, ancestors=True, _reserved=0):
        """vdjx_tree_spr: tree_mp() with subtree pruning and regrafting as the rearrangement -- inside every clone of four and more, rounds
        that score every (pruned node, edge to regraft it on) and apply the best while it lowers the Fitch total, from tree_nj's tree
        (start=None) or from the caller's (start: int32[nodes], parents in tree_nj's slots); max_rounds caps a lineage's scoring rounds
        (0: until no move lowers the total).  Arguments and result as tree_mp()'s -> {"parent", "mutations", "depth", "clone" int32:
        [nodes] each, "anc": the inferred nodes' windows as str (None with ancestors=False), "info": dict(TREE_SPR_FIELDS)}; a lineage of
        more than 1,024 members is refused."""
        raw, n, ln = self._contig_block(contigs, "vdjx_tree_spr")
        cl = np.ascontiguousarray(clone, np.int32)
        an = np.ascontiguousarray(anchor, np.int32)
        pr = None if prio is None else np.ascontiguousarray(prio, np.uint32)
        if cl.shape != (n,) or an.shape != (n,) or (pr is not None and pr.shape != (n,)):
            raise VdjxError(f"vdjx_tree_spr: {n} contigs, clone of shape {cl.shape}, anchor of shape {an.shape}")
        total = C.c_uint64(0)
        check(self.L.vdjx_tree_nj_nodes(_p(cl), n, C.byref(total)), "vdjx_tree_nj_nodes")
        nodes = int(total.value)
        sp = None if start is None else np.ascontiguousarray(start, np.int32)
        if sp is not None and sp.shape != (nodes,):
            raise VdjxError(f"vdjx_tree_spr: start of shape {sp.shape} for {nodes} nodes")
        if not 0 <= int(max_rounds) < 1 << 32:
            raise VdjxError(f"vdjx_tree_spr: max_rounds {max_rounds}")
        params = _lib.TreeSprParams(int(max_rounds), int(_reserved))
        parent, mutations, depth, out_clone = (np.zeros(nodes, np.int32) for _ in range(4))
        anc = np.zeros((nodes - n, max(ln, 1)), np.uint8) if ancestors else None
        info = _lib.TreeSprInfo()
        check(self.L.vdjx_tree_spr(self.h, raw, n, ln, _p(cl), _p(an), _p(pr), _p(sp), C.byref(params), _p(parent), _p(mutations), _p(depth),
                                   _p(out_clone), _p(anc), C.byref(info)), "vdjx_tree_spr")
        return {"parent": parent, "mutations": mutations, "depth": depth, "clone": out_clone,
                "anc": None if anc is None else [row.tobytes().split(b"\0", 1)[0].decode("latin-1") for row in anc],
                "info": {f: int(getattr(info, f)) for f in self.TREE_SPR_FIELDS}}

    TREE_SANKOFF_FIELDS = ("members", "clones", "largest_clone", "internal", "batches", "searched", "moved", "rounds", "edges", "moves",
                           "candidates", "cost_start", "cost", "mutations")

    def tree_sankoff(self, contigs, clone, anchor, prio=None, cost=None, start=None, search=True, max_rounds=0, ancestors=True, _reserved=0):
        """vdjx_tree_sankoff: tree_mp() under a cost matrix -- cost: uint32[4, 4], cost[s][t] the price of a parent in state s over a child
        in state t (A C G T; the diagonal 0, the rest 1 .. 65535; None: all 1, Fitch's count; annot.sankoff_costs makes one from a targeting
        model).  Inside every clone the weighted cost of tree_nj's tree (start=None) or of the caller's (start: int32[nodes], parents in
        tree_nj's slots), with search the rounds of nearest-neighbour interchanges that lower it (max_rounds caps a lineage's rounds, 0:
        until none does), then Sankoff's down pass.  -> {"parent", "mutations", "depth", "clone" int32, "cost" int64: [nodes] each, in
        tree_nj's slots (a root has parent -1, cost -1 and mutations -1), "anc": the inferred nodes' windows as str (None with
        ancestors=False), "info": dict(TREE_SANKOFF_FIELDS)}."""
        raw, n, ln = self._contig_block(contigs, "vdjx_tree_sankoff")
        cl = np.ascontiguousarray(clone, np.int32)
        an = np.ascontiguousarray(anchor, np.int32)
        pr = None if prio is None else np.ascontiguousarray(prio, np.uint32)
        if cl.shape != (n,) or an.shape != (n,) or (pr is not None and pr.shape != (n,)):
            raise VdjxError(f"vdjx_tree_sankoff: {n} contigs, clone of shape {cl.shape}, anchor of shape {an.shape}")
        co = None
        if cost is not None:
            given = np.asarray(cost)
            if given.shape != (4, 4) or given.dtype.kind not in "ui" or (given < 0).any() or (given >= 1 << 32).any():
                raise VdjxError(f"vdjx_tree_sankoff: cost of shape {given.shape} and type {given.dtype}: whole numbers below 2^32, [4, 4]")
            co = np.ascontiguousarray(given, np.uint32)
        total = C.c_uint64(0)
        check(self.L.vdjx_tree_nj_nodes(_p(cl), n, C.byref(total)), "vdjx_tree_nj_nodes")
        nodes = int(total.value)
        sp = None if start is None else np.ascontiguousarray(start, np.int32)
        if sp is not None and sp.shape != (nodes,):
            raise VdjxError(f"vdjx_tree_sankoff: start of shape {sp.shape} for {nodes} nodes")
        if not 0 <= int(max_rounds) < 1 << 32 or not 0 <= int(search) < 1 << 32:
            raise VdjxError(f"vdjx_tree_sankoff: max_rounds {max_rounds}, search {search}")
        params = _lib.TreeSankoffParams(int(max_rounds), int(search), (C.c_uint32 * 2)(int(_reserved), 0))
        parent, mutations, depth, out_clone = (np.zeros(nodes, np.int32) for _ in range(4))
        out_cost = np.zeros(nodes, np.int64)
        anc = np.zeros((nodes - n, max(ln, 1)), np.uint8) if ancestors else None
        info = _lib.TreeSankoffInfo()
        check(self.L.vdjx_tree_sankoff(self.h, raw, n, ln, _p(cl), _p(an), _p(pr), _p(co), _p(sp), C.byref(params), _p(parent), _p(out_cost),
                                       _p(mutations), _p(depth), _p(out_clone), _p(anc), C.byref(info)), "vdjx_tree_sankoff")
        return {"parent": parent, "cost": out_cost, "mutations": mutations, "depth": depth, "clone": out_clone,
                "anc": None if anc is None else [row.tobytes().split(b"\0", 1)[0].decode("latin-1") for row in anc],
                "info": {f: int(getattr(info, f)) for f in self.TREE_SANKOFF_FIELDS}}

    def tree_sankoff_spr(self, contigs, clone, anchor, prio=None, cost=None, start=None, max_rounds=0, ancestors=True, _reserved=0):
        """vdjx_tree_sankoff_spr: tree_spr()'s search under tree_sankoff()'s cost -- inside every clone of four and more, rounds that score
        every (pruned node, edge to regraft it on) under cost (uint32[4, 4] as tree_sankoff() takes it; None: all 1) and apply the best
        while it lowers the weighted total, from tree_nj's tree (start=None) or from the caller's (start: int32[nodes], parents in
        tree_nj's slots); max_rounds caps a lineage's scoring rounds (0: until no move lowers the total); then Sankoff's down pass.
        -> tree_sankoff()'s dict; info["candidates"] counts as tree_spr()'s.  A lineage of more than 1,024 members is refused."""
        raw, n, ln = self._contig_block(contigs, "vdjx_tree_sankoff_spr")
        cl = np.ascontiguousarray(clone, np.int32)
        an = np.ascontiguousarray(anchor, np.int32)
        pr = None if prio is None else np.ascontiguousarray(prio, np.uint32)
        if cl.shape != (n,) or an.shape != (n,) or (pr is not None and pr.shape != (n,)):
            raise VdjxError(f"vdjx_tree_sankoff_spr: {n} contigs, clone of shape {cl.shape}, anchor of shape {an.shape}")
        co = None
        if cost is not None:
            given = np.asarray(cost)
            if given.shape != (4, 4) or given.dtype.kind not in "ui" or (given < 0).any() or (given >= 1 << 32).any():
                raise VdjxError(f"vdjx_tree_sankoff_spr: cost of shape {given.shape} and type {given.dtype}: whole numbers below 2^32, [4, 4]")
            co = np.ascontiguousarray(given, np.uint32)
        total = C.c_uint64(0)
        check(self.L.vdjx_tree_nj_nodes(_p(cl), n, C.byref(total)), "vdjx_tree_nj_nodes")
        nodes = int(total.value)
        sp = None if start is None else np.ascontiguousarray(start, np.int32)
        if sp is not None and sp.shape != (nodes,):
            raise VdjxError(f"vdjx_tree_sankoff_spr: start of shape {sp.shape} for {nodes} nodes")
        if not 0 <= int(max_rounds) < 1 << 32:
            raise VdjxError(f"vdjx_tree_sankoff_spr: max_rounds {max_rounds}")
        params = _lib.TreeSankoffSprParams(int(max_rounds), (C.c_uint32 * 3)(int(_reserved), 0, 0))
        parent, mutations, depth, out_clone = (np.zeros(nodes, np.int32) for _ in range(4))
        out_cost = np.zeros(nodes, np.int64)
        anc = np.zeros((nodes - n, max(ln, 1)), np.uint8) if ancestors else None
        info = _lib.TreeSankoffInfo()
        check(self.L.vdjx_tree_sankoff_spr(self.h, raw, n, ln, _p(cl), _p(an), _p(pr), _p(co), _p(sp), C.byref(params), _p(parent), _p(out_cost),
                                           _p(mutations), _p(depth), _p(out_clone), _p(anc), C.byref(info)), "vdjx_tree_sankoff_spr")
        return {"parent": parent, "cost": out_cost, "mutations": mutations, "depth": depth, "clone": out_clone,
                "anc": None if anc is None else [row.tobytes().split(b"\0", 1)[0].decode("latin-1") for row in anc],
                "info": {f: int(getattr(info, f)) for f in self.TREE_SANKOFF_FIELDS}}

    TREE_SPLIT_FIELDS = ("members", "clones", "largest_clone", "replicates", "batches", "units", "scored", "matched", "full", "joins", "cells")

    def tree_split_support(self, contigs, clone, anchor, parent, prio=None, replicates=100, seed=1, return_trees=False, _reserved=0):
        """vdjx_tree_split_support: the delete-half jackknife around neighbour joining.  contigs, clone, anchor, prio as tree_nj() takes
        them; parent: int32[nodes] in tree_nj's slots, the scored tree (tree_nj's or tree_mp's "parent", or any tree tree_mp takes as a
        start); replicates: 1 .. 1024; seed: any uint64 (tree_support's keep rule) -> {"support": int32[nodes] (for an inferred node other
        than a root's child, in a lineage of four and more: the replicates whose neighbour-joining tree has its split; -1 elsewhere),
        "trees": int32[replicates, nodes] (every replicate's parents in tree_nj's slots; None unless return_trees), "info":
        dict(TREE_SPLIT_FIELDS)}"""
        raw, n, ln = self._contig_block(contigs, "vdjx_tree_split_support")
        cl = np.ascontiguousarray(clone, np.int32)
        an = np.ascontiguousarray(anchor, np.int32)
        pr = None if prio is None else np.ascontiguousarray(prio, np.uint32)
        if cl.shape != (n,) or an.shape != (n,) or (pr is not None and pr.shape != (n,)):
            raise VdjxError(f"vdjx_tree_split_support: {n} contigs, clone of shape {cl.shape}, anchor of shape {an.shape}")
        total = C.c_uint64(0)
        check(self.L.vdjx_tree_nj_nodes(_p(cl), n, C.byref(total)), "vdjx_tree_nj_nodes")
        nodes = int(total.value)
        pa = np.ascontiguousarray(parent, np.int32)
        if pa.shape != (nodes,):
            raise VdjxError(f"vdjx_tree_split_support: parent of shape {pa.shape} for {nodes} nodes")
        if not 0 <= int(replicates) < 1 << 32 or not 0 <= int(seed) < 1 << 64:
            raise VdjxError(f"vdjx_tree_split_support: replicates {replicates}, seed {seed}")
        b = int(replicates)
        params = _lib.TreeSplitParams(b, int(_reserved), int(seed))
        support = np.zeros(nodes, np.int32)
        trees = np.zeros((b if 1 <= b <= 1024 else 1, nodes), np.int32) if return_trees else None      # (a count the library refuses: nothing is written)
        info = _lib.TreeSplitInfo()
        check(self.L.vdjx_tree_split_support(self.h, raw, n, ln, _p(cl), _p(an), _p(pr), _p(pa), C.byref(params), _p(support), _p(trees), C.byref(info)),
              "vdjx_tree_split_support")
        return {"support": support, "trees": trees, "info": {f: int(getattr(info, f)) for f in self.TREE_SPLIT_FIELDS}}

    DIVERSITY_FIELDS = ("clones", "weighted", "weight", "depth", "replicates", "batches", "path")

    def diversity(self, weight, depth, q=None, replicates=200, seed=1, counts=False):
        """vdjx_diversity: the Hill curve of the clone abundances, bootstrapped.  weight: uint64[C], the abundance of every clone in any unit
        (0 is legal: never drawn); depth: the draws of a replicate, 1 .. 2^31 - 1; q: the orders, float64[Q] (None: annot.diversity_orders(),
        0.0 .. 4.0 in tenths); replicates: 1 .. 4096; seed: any uint64 -> {"observed", "mean", "sd": float64[Q], "d": float64[B, Q],
        "counts": uint32[B, C] (None unless counts=True), "info": dict(clones, weighted, weight, depth, replicates, batches, path)}"""
        from . import annot
        w = np.ascontiguousarray(weight, np.uint64)
        qs = np.ascontiguousarray(annot.diversity_orders() if q is None else q, np.float64)
        if w.ndim != 1 or qs.ndim != 1:
            raise VdjxError(f"vdjx_diversity: weight of shape {w.shape}, q of shape {qs.shape}")
        if not 0 <= int(replicates) < 1 << 32 or not 0 <= int(depth) < 1 << 32 or not 0 <= int(seed) < 1 << 64:
            raise VdjxError(f"vdjx_diversity: replicates {replicates}, depth {depth}, seed {seed}")
        n, nq, b = w.shape[0], qs.shape[0], int(replicates)
        rows = b if 1 <= b <= 4096 else 1                                 # (a count the library refuses: nothing is written)
        params = _lib.DiversityParams(b, int(depth), int(seed))
        observed, mean, sd = np.zeros(nq), np.zeros(nq), np.zeros(nq)
        d = np.zeros((rows, nq))
        cnt = np.zeros((rows, n), np.uint32) if counts else None
        info = _lib.DiversityInfo()
        check(self.L.vdjx_diversity(self.h, _p(w), n, _p(qs), nq, C.byref(params), _p(observed), _p(d), _p(mean), _p(sd), _p(cnt), C.byref(info)),
              "vdjx_diversity")
        return {"observed": observed, "mean": mean, "sd": sd, "d": d, "counts": cnt, "info": {f: int(getattr(info, f)) for f in self.DIVERSITY_FIELDS}}

    def stat(self, name: str) -> int:
        return int(self.L.vdjx_stat(self.h, name.encode()))

    # ---- profiling
    def profile(self, on: bool = True):
        check(self.L.vdjx_profile_enable(self.h, 1 if on else 0))

    def profile_only(self, name=None) -> None:
        """bracket only the launches of this scope from now on (None: all again)"""
        check(self.L.vdjx_profile_only(self.h, name.encode() if name else None), "vdjx_profile_only")

    def profile_reset(self):
        check(self.L.vdjx_profile_reset(self.h))

    def profile_get(self) -> dict:
        out = {}
        n = self.L.vdjx_profile_count(self.h)
        for i in range(n):
            name = C.c_char_p()
            ms = C.c_double()
            cnt = C.c_uint64()
            check(self.L.vdjx_profile_get(self.h, i, C.byref(name), C.byref(ms), C.byref(cnt)))
            out[name.value.decode()] = (ms.value, int(cnt.value))
        return out


def sam_text(pool_np, names, contig_ids, offsets, pairs, rl: int) -> str:
    """SAM records of quick_map3.c:152-181 from map_emit's pairs (host formatting; text only)."""
    pri, sec = pool_np
    npri = pri.shape[0]

    def rec(r):
        row = pri[r] if r < npri else sec[r - npri]
        return row[1:1 + rl].tobytes().decode(), row[1 + rl:1 + 2 * rl].tobytes().decode()

    out = []
    for ci, cid in enumerate(contig_ids):
        for q in pairs[int(offsets[ci]):int(offsets[ci + 1])]:
            name = names[int(q["pair_id"])]
            if name.startswith("@"):
                name = name[1:]
            f1 = 1 | 2 | (0x10 if q["rc1"] else 0x20) | 0x40
            f2 = 1 | 2 | (0x10 if q["rc2"] else 0x20) | 0x80
            s1, q1 = rec(int(q["rec1"]))
            s2, q2 = rec(int(q["rec2"]))
            out.append(f"{name}\t{f1}\t{cid}\t{q['pos1']}\t255\t{rl}M\t=\t{q['pos2']}\t{q['insert']}\t{s1}\t{q1}\n")
            out.append(f"{name}\t{f2}\t{cid}\t{q['pos2']}\t255\t{rl}M\t=\t{q['pos1']}\t{q['insert']}\t{s2}\t{q2}\n")
    return "".join(out)
