"""Host-side mirror of the reference's seams for the SEARCH_GG path, over the C-ABI.

    CtrDB.open(path)                 ~ UTree *XT_read32(char *db, ';')                   itree.c:733
    DeviceTree.upload(db, device)    ~ the UTree's Dump/BinIx made resident in HBM       itree.c:140-141
    tree.get_ix(words)               ~ IXTYPE XT_getIX32(UTree*, WTYPE word)             itree.c:720
    tree.classify(bases, off, len)   ~ the per-read body of XT_doSearch32, GG branch     itree.c:891-1088
    search_gg(db, trees, in, out)    ~ size_t XT_doSearch32(utree, in, out, 8, 0, doRC)  itree.c:833
    search_gg(..., mates=, interleaved=)   the same over paired-end reads: both mates of a pair cast one vote
    tree.join_pairs(...)             the device join in front of classify(): mate 1 + 'N' + mate 2 per pair
    tree.profile(capacity)           per-taxon read counts of classified batches (no counterpart in the reference)
    tree.coverage()                  per-taxon database k-mers, distinct ones hit, hits (no counterpart in the reference)
    tree.samples()                   per-sample taxon table of multiplexed reads, ids interned on the device (no counterpart in the reference)
    tree.sample_redistribution()     ambiguous reads of multiplexed reads redistributed within each sample (no counterpart in the reference)
    tree.tiles_plan / tiles_views    the tiles of long queries as views into their bases, for classify() (no counterpart in the reference)
    tiles_file(db, tree, in, ...)    the `utree-tiles` run: tiles.tsv and segments.tsv of a file of long queries
    tree.redistribution()            candidate sets of ambiguous reads, redistributed among their tied labels (as xtree does)

torch is used only for device memory and streams (plumbing); every computation happens in the HIP kernels
behind libutree_amd.so.  Nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import lib as _lib

RESULT_FIELDS = ("label", "cut", "found", "uix", "sl", "ol")
RESULT_DTYPE = np.dtype([("label", "<u4"), ("cut", "<i4"), ("found", "<u4"), ("uix", "<u4"), ("sl", "<u4"),
                         ("ol", "<u4")])
PROFILE_ENTRY_DTYPE = np.dtype([("label", "<u4"), ("cut", "<i4"), ("reads", "<u8")])
COVERAGE_ENTRY_DTYPE = np.dtype([("label", "<u4"), ("pad", "<u4"), ("db_kmers", "<u8"), ("covered", "<u8"), ("hits", "<u8")])
REDIST_SET_DTYPE = np.dtype([("reads", "<u8"), ("first", "<u8"), ("n", "<u4"), ("pad", "<u4")])
REDIST_ENTRY_DTYPE = np.dtype([("label", "<u4"), ("pad", "<u4"), ("assigned", "<u8"), ("unique", "<u8")])
SREDIST_CELL_DTYPE = np.dtype([("sample", "<u4"), ("n", "<u4"), ("first", "<u8"), ("reads", "<u8")])
SREDIST_ENTRY_DTYPE = np.dtype([("sample", "<u4"), ("label", "<u4"), ("assigned", "<u8"), ("unique", "<u8")])
SAMPLES_CELL_DTYPE = np.dtype([("sample", "<u4"), ("label", "<u4"), ("cut", "<i4"), ("pad", "<u4"), ("reads", "<u8")])


class CtrDB:
    """Host side of a `.ctr` database: header, bin table, labels (XT_read32, itree.c:733-828)."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        info = _lib.CtrInfo()
        _lib.check(_lib.load().utree_ctr_get_info(self._h, C.byref(info)), "utree_ctr_get_info")
        self.info = info

    @classmethod
    def open(cls, path: str) -> "CtrDB":
        h = C.c_void_p()
        _lib.check(_lib.load().utree_ctr_open(path.encode(), C.byref(h)), "utree_ctr_open(%s)" % path)
        return cls(h.value)

    @classmethod
    def from_memory(cls, W: int, I: int, n_nodes: int, binix: np.ndarray, records: Optional[np.ndarray],
                    label_text: bytes) -> "CtrDB":
        width = 4 if n_nodes < 0xFFFFFFFF else 8
        b = np.ascontiguousarray(binix.astype("<u4" if width == 4 else "<u8"))
        rec_ptr = None
        if records is not None:
            records = np.ascontiguousarray(records, dtype=np.uint8)
            rec_ptr = records.ctypes.data
        h = C.c_void_p()
        _lib.check(_lib.load().utree_ctr_from_memory(W, I, n_nodes, b.ctypes.data, width, rec_ptr, label_text,
                                                     len(label_text), C.byref(h)), "utree_ctr_from_memory")
        return cls(h.value)

    W = property(lambda s: s.info.W)
    I = property(lambda s: s.info.I)
    k = property(lambda s: s.info.k)
    n_nodes = property(lambda s: s.info.n_nodes)
    n_labels = property(lambda s: s.info.n_labels)

    def label(self, ix: int) -> Optional[bytes]:
        n = C.c_uint32()
        p = _lib.load().utree_ctr_label(self._h, ix, C.byref(n))
        return None if not p else C.string_at(p, n.value)

    def format(self, buf: np.ndarray, name_off: np.ndarray, name_len: np.ndarray, results: np.ndarray,
               rank: bool = False) -> bytes:
        """Output lines of itree.c:1032/1040/1096 for framed reads and their results (rank=True: the
        rank-specific search's lines, itree.c:1002)."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        name_len = np.ascontiguousarray(name_len, dtype=np.uint32)
        results = np.ascontiguousarray(results)
        assert results.dtype.itemsize == 24 or results.dtype == np.int32
        n = len(name_off)
        cap = int(name_len.sum()) + n * 256 + 4096
        bad = C.c_size_t(-1).value
        while True:
            out = np.empty(cap, dtype=np.uint8)
            good = C.c_uint64(0)
            fn = _lib.load().utree_format_rank_records if rank else _lib.load().utree_format_records
            L = fn(self._h, buf.ctypes.data, name_off.ctypes.data, name_len.ctypes.data,
                   results.ctypes.data, n, out.ctypes.data, cap, C.byref(good))
            if L != bad:
                break
            if cap > (1 << 34):
                raise _lib.UtreeError(_lib.E_NOMEM, "utree_format_records")
            cap *= 4
        return out[:L].tobytes()

    def close(self):
        if self._h:
            _lib.load().utree_ctr_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frame_fasta(data: bytes, final: bool = True):
    """a2: frame reads as the reference's two fgets per read do (itree.c:866-890)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    cap = max(1, data.count(b"\n") // 2 + 2)
    seq_off = np.zeros(cap, dtype=np.uint64)
    seq_len = np.zeros(cap, dtype=np.uint32)
    name_off = np.zeros(cap, dtype=np.uint64)
    name_len = np.zeros(cap, dtype=np.uint32)
    n = C.c_size_t(0)
    used = C.c_size_t(0)
    err = _lib.FastaError()
    rc = _lib.load().utree_fasta_frame(buf.ctypes.data if len(buf) else None, len(buf), int(final), cap,
                                       seq_off.ctypes.data, seq_len.ctypes.data, name_off.ctypes.data,
                                       name_len.ctypes.data, C.byref(n), C.byref(used), C.byref(err))
    if rc not in (_lib.OK, _lib.E_FASTA):
        _lib.check(rc, "utree_fasta_frame")
    k = n.value
    return dict(seq_off=seq_off[:k], seq_len=seq_len[:k], name_off=name_off[:k], name_len=name_len[:k],
                consumed=used.value, error_code=err.code if rc else 0, error_read=err.read_index)


def frame_reads(data: bytes, fmt: int, final: bool = True):
    """Opt-in input formats (FASTQ, multi-line FASTA).  Returns the framing AND the buffer: multi-line
    sequences are compacted in place, so offsets refer to the returned array, not to `data`."""
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    cap = max(1, data.count(b"\n") + 2)
    seq_off = np.zeros(cap, dtype=np.uint64)
    seq_len = np.zeros(cap, dtype=np.uint32)
    name_off = np.zeros(cap, dtype=np.uint64)
    name_len = np.zeros(cap, dtype=np.uint32)
    n = C.c_size_t(0)
    used = C.c_size_t(0)
    err = _lib.FastaError()
    rc = _lib.load().utree_reads_frame(buf.ctypes.data if len(buf) else None, len(buf), int(final), fmt, cap,
                                       seq_off.ctypes.data, seq_len.ctypes.data, name_off.ctypes.data,
                                       name_len.ctypes.data, C.byref(n), C.byref(used), C.byref(err))
    if rc not in (_lib.OK, _lib.E_FASTA):
        _lib.check(rc, "utree_reads_frame")
    k = n.value
    return dict(buf=buf, seq_off=seq_off[:k], seq_len=seq_len[:k], name_off=name_off[:k], name_len=name_len[:k],
                consumed=used.value, error_code=err.code if rc else 0, error_read=err.read_index)


class DeviceTree:
    """The database resident in one GPU's HBM (device image)."""

    def __init__(self, handle, db: CtrDB, keepalive=None):
        self._h = C.c_void_p(handle)
        self.db = db
        self._keep = keepalive
        info = _lib.DevInfo()
        _lib.check(_lib.load().utree_dev_get_info(self._h, C.byref(info)), "utree_dev_get_info")
        self.info = info
        self._ws = None

    @classmethod
    def upload(cls, db: CtrDB, device: int = 0, fine_bits: int = _lib.FINE_AUTO) -> "DeviceTree":
        h = C.c_void_p()
        _lib.check(_lib.load().utree_dev_upload(db._h, device, fine_bits, C.byref(h)), "utree_dev_upload")
        return cls(h.value, db)

    @classmethod
    def build_from_device(cls, db: CtrDB, d_binix, d_records, device: int = 0, fine_bits: int = _lib.FINE_AUTO,
                          image=None) -> "DeviceTree":
        """d_binix / d_records: torch uint8 CUDA tensors holding the on-disk bin table and node dump."""
        import torch
        L = _lib.load()
        need = L.utree_dev_image_bytes(db._h, fine_bits)
        if image is None:
            image = torch.empty(need, dtype=torch.uint8, device="cuda:%d" % device)
        assert image.numel() >= need and image.is_cuda
        h = C.c_void_p()
        stream = torch.cuda.current_stream(device).cuda_stream
        _lib.check(L.utree_dev_build(db._h, device, fine_bits, d_binix.data_ptr(), d_records.data_ptr(), image.data_ptr(),
                                     image.numel(), stream, C.byref(h)), "utree_dev_build")
        return cls(h.value, db, keepalive=image)

    @classmethod
    def attach(cls, db: CtrDB, image, device: int) -> "DeviceTree":
        """Adopt an image received by torch.distributed.broadcast (RCCL) on this rank's GPU."""
        h = C.c_void_p()
        _lib.check(_lib.load().utree_dev_attach(db._h, device, image.data_ptr(), image.numel(), C.byref(h)),
                   "utree_dev_attach")
        return cls(h.value, db, keepalive=image)

    @staticmethod
    def rccl_unique_id() -> bytes:
        """Root side of the one-process-per-GPU replication: the id every rank's communicator is built from."""
        buf = C.create_string_buffer(128)
        _lib.check(_lib.load().utree_rccl_unique_id(buf, 128), "utree_rccl_unique_id")
        return buf.raw

    @classmethod
    def replicate_rank(cls, db: Optional[CtrDB], tree: Optional["DeviceTree"], device: int, rank: int, world: int, root: int,
                       uid: bytes) -> "DeviceTree":
        """utree_dev_replicate_rank: ONE ncclBroadcast (RCCL over xGMI) of the root's flat image issued from C; the root
        passes its tree and gets it back, the others pass tree=None and get a handle that owns the received copy."""
        h = C.c_void_p()
        _lib.check(_lib.load().utree_dev_replicate_rank(db._h if db is not None else None, tree._h if tree is not None else None,
                                                        device, rank, world, root, uid, len(uid), C.byref(h)),
                   "utree_dev_replicate_rank")
        if tree is not None and h.value == tree._h.value:
            return tree
        return cls(h.value, db if db is not None else (tree.db if tree is not None else None))   # a received copy (root: only under UTREE_RCCL_FORCE)

    @classmethod
    def replicate(cls, db: CtrDB, tree: "DeviceTree", devices) -> list:
        """utree_dev_replicate: one process, the image broadcast to `devices` (devices[0] = the tree's own).  Returns the handles;
        [0] is `tree` itself unless UTREE_RCCL_FORCE made it a replica on the same card."""
        n = len(devices)
        arr = (C.c_int * n)(*devices)
        out = (C.c_void_p * n)()
        _lib.check(_lib.load().utree_dev_replicate(db._h, tree._h, arr, n, out), "utree_dev_replicate")
        return [tree if out[i] == tree._h.value else cls(out[i], db) for i in range(n)]

    @staticmethod
    def replicate_seconds() -> float:
        return float(_lib.load().utree_dev_replicate_seconds())

    def image_tensor(self):
        """The flat image as a torch uint8 tensor view (for broadcast); only when torch owns the memory."""
        return self._keep

    def image_ptr(self):
        p = C.c_void_p()
        n = C.c_size_t()
        _lib.check(_lib.load().utree_dev_image(self._h, C.byref(p), C.byref(n)), "utree_dev_image")
        return p.value, n.value

    def get_ix(self, hi, lo):
        """XT_getIX32 (itree.c:720) for a batch of words. hi/lo: torch int64 CUDA tensors (hi may be None for k=32)."""
        import torch
        n = lo.numel()
        out = torch.empty(n, dtype=torch.int32, device=lo.device)
        stream = torch.cuda.current_stream(lo.device).cuda_stream
        _lib.check(_lib.load().utree_lookup_words(self._h, hi.data_ptr() if hi is not None else None, lo.data_ptr(), n,
                                                  out.data_ptr(), stream), "utree_lookup_words")
        return out

    def workspace_bytes(self, n_reads: int, total_bases: int, max_len: int, rc: bool) -> int:
        return _lib.load().utree_classify_workspace_bytes(self._h, n_reads, total_bases, max_len, int(rc))

    def classify(self, bases, off, length, rc: bool = False, total_bases: Optional[int] = None,
                 max_len: Optional[int] = None, out=None, workspace=None):
        """The hot path for one batch (a3-a9). bases: uint8 CUDA tensor; off: int64; length: int32.
        Returns an int32 [n, 6] CUDA tensor (label, cut, found, uix, sl, ol). Asynchronous on torch's
        current stream."""
        import torch
        n = off.numel()
        dev = bases.device
        if total_bases is None:
            total_bases = int(length.sum().item())
        if max_len is None:
            max_len = int(length.max().item()) if n else 0
        if out is None:
            out = torch.empty((n, 6), dtype=torch.int32, device=dev)
        need = self.workspace_bytes(n, total_bases, max_len, rc)
        if workspace is None:
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = self._ws
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().utree_classify_batch(self._h, bases.data_ptr(), off.data_ptr(), length.data_ptr(), n,
                                                    total_bases, max_len, int(rc), out.data_ptr(), workspace.data_ptr(),
                                                    workspace.numel(), stream), "utree_classify_batch")
        return out

    def join_pairs(self, bases1, off1, len1, bases2, off2, len2, capacity: Optional[int] = None):
        """utree_pairs_join: per pair mate 1 + 'N' + mate 2 as one query.  Mates as classify() takes reads (uint8 / int64 / int32 CUDA tensors,
        any alignment and order; both may lie in one buffer).  capacity: bytes of the joined buffer (default: total1 + total2 + pairs).
        Returns (joined, joff, jlen, meta): uint8 [capacity], int64 [n] and int32 [n] CUDA tensors for classify(), and meta = the dict
        {total_bases, max_len, error} read back once the stream has drained (error != 0: capacity too small or a pair too long -- nothing
        was joined)."""
        import torch
        dev = self.info.device
        for t, dt in ((bases1, torch.uint8), (off1, torch.int64), (len1, torch.int32), (bases2, torch.uint8), (off2, torch.int64), (len2, torch.int32)):
            if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous() and t.is_cuda and t.device.index == dev):
                raise ValueError("join_pairs: bases / off / len must be contiguous uint8 / int64 / int32 tensors on cuda:%d" % dev)
        n = off1.numel()
        if not (len1.numel() == off2.numel() == len2.numel() == n):
            raise ValueError("join_pairs: the four offset and length tensors must have one entry per pair")
        if capacity is None:
            capacity = int(len1.sum().item()) + int(len2.sum().item()) + n
        joined = torch.empty(capacity, dtype=torch.uint8, device=bases1.device)
        joff = torch.empty(n, dtype=torch.int64, device=bases1.device)
        jlen = torch.empty(n, dtype=torch.int32, device=bases1.device)
        d_meta = torch.zeros(2, dtype=torch.int64, device=bases1.device)
        stream = torch.cuda.current_stream(bases1.device)
        _lib.check(_lib.load().utree_pairs_join(self._h, bases1.data_ptr(), off1.data_ptr(), len1.data_ptr(), bases2.data_ptr(), off2.data_ptr(),
                                                len2.data_ptr(), n, joined.data_ptr(), capacity, joff.data_ptr(), jlen.data_ptr(),
                                                d_meta.data_ptr(), stream.cuda_stream), "utree_pairs_join")
        stream.synchronize()
        m = _lib.PairsMeta.from_buffer_copy(d_meta.cpu().numpy().tobytes())
        return joined, joff, jlen, dict(total_bases=int(m.total_bases), max_len=int(m.max_len), error=int(m.error))

    def hitmap(self, bases, off, length, rc: bool = False, capacity: Optional[int] = None, total_bases: Optional[int] = None,
               runs=None, workspace=None, sync: bool = True):
        """utree_hitmap_batch: which label each k-mer window of each query hit, in window order, as runs.  Reads as classify() takes them
        (pairs: join_pairs first).  capacity: entries of the runs tensor (default: one per window, which always suffices); runs: a
        [>= capacity, 2] int32 tensor to write into.  Returns (run_off, runs, meta): int64 [n + 1], int32 [capacity, 2] of (code, count) --
        read r's runs are runs[run_off[r]:run_off[r + 1]], codes HIT_MISS / HIT_INVALID read as -1 / -2 -- and meta = the dict {total_runs,
        total_windows, error} read back once the stream has drained (error 1: capacity < total_runs, nothing at or beyond it was written).
        sync=False: the call returns at once (asynchronous on torch's current stream, workspace= the caller's own) and meta is the int64 [3]
        device tensor (total_runs, total_windows, error)."""
        import torch
        n = off.numel()
        dev = bases.device
        if total_bases is None:
            total_bases = int(length.sum().item()) if n else 0
        need = _lib.load().utree_hitmap_workspace_bytes(self._h, n, total_bases, int(rc))
        if not need:
            raise _lib.UtreeError(_lib.E_ARG, "utree_hitmap_workspace_bytes")
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        if capacity is None:
            capacity = 2 * total_bases + n if rc else total_bases
        if runs is None:
            runs = torch.empty((max(capacity, 1), 2), dtype=torch.int32, device=dev)
        assert runs.numel() >= 2 * capacity and runs.is_contiguous() and workspace.numel() >= need
        run_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_meta = torch.zeros(3, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev)
        _lib.check(_lib.load().utree_hitmap_batch(self._h, bases.data_ptr(), off.data_ptr(), length.data_ptr(), n, total_bases, int(rc),
                                                  run_off.data_ptr(), runs.data_ptr(), capacity, d_meta.data_ptr(), workspace.data_ptr(),
                                                  workspace.numel(), stream.cuda_stream), "utree_hitmap_batch")
        if not sync:
            return run_off, runs, d_meta
        stream.synchronize()
        m = _lib.HitmapMeta.from_buffer_copy(d_meta.cpu().numpy().tobytes())
        return run_off, runs, dict(total_runs=int(m.total_runs), total_windows=int(m.total_windows), error=int(m.error))

    def tiles_plan(self, length, tile_bp: int, step_bp: int):
        """utree_tiles_plan: the tiles of a batch of queries, W = tile_bp, S = step_bp.  length: int32 CUDA tensor of the queries' lengths.
        Returns (tile_first, meta): the int64 [n + 1] CUDA tensor of the tiles in front of each query (the last entry is the batch's total)
        and meta = the dict {total_tiles, total_bases, max_len, error} read back once the stream has drained."""
        import torch
        n = length.numel()
        dev = length.device
        need = _lib.load().utree_tiles_workspace_bytes(self._h, n)
        if not need:
            raise _lib.UtreeError(_lib.E_ARG, "utree_tiles_workspace_bytes")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        tile_first = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_meta = torch.zeros(3, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev)
        _lib.check(_lib.load().utree_tiles_plan(self._h, length.data_ptr(), n, tile_bp, step_bp, tile_first.data_ptr(), d_meta.data_ptr(),
                                                ws.data_ptr(), ws.numel(), stream.cuda_stream), "utree_tiles_plan")
        stream.synchronize()
        return tile_first, _tiles_meta(d_meta)

    def tiles_views(self, off, length, tile_bp: int, step_bp: int, tile_first, first_tile: int, n_tiles: int):
        """utree_tiles_views: tiles [first_tile, first_tile + n_tiles) of the plan `tile_first` as views into the queries' bases.  off /
        length: the queries as classify() takes them.  Returns (toff, tlen, tquery, tindex, meta): int64 / int32 / int32 / int32 CUDA
        tensors of n_tiles entries -- classify(bases, toff, tlen, total_bases=meta["total_bases"], max_len=meta["max_len"]) classifies the
        tiles -- and meta as tiles_plan gives it (error 1: the range ends behind the plan's tiles, nothing was written)."""
        import torch
        dev = tile_first.device
        toff = torch.empty(n_tiles, dtype=torch.int64, device=dev)
        tlen = torch.empty(n_tiles, dtype=torch.int32, device=dev)
        tquery = torch.empty(n_tiles, dtype=torch.int32, device=dev)
        tindex = torch.empty(n_tiles, dtype=torch.int32, device=dev)
        d_meta = torch.zeros(3, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev)
        _lib.check(_lib.load().utree_tiles_views(self._h, off.data_ptr(), length.data_ptr(), length.numel(), tile_bp, step_bp, tile_first.data_ptr(),
                                                 first_tile, n_tiles, toff.data_ptr(), tlen.data_ptr(), tquery.data_ptr(), tindex.data_ptr(),
                                                 d_meta.data_ptr(), stream.cuda_stream), "utree_tiles_views")
        stream.synchronize()
        return toff, tlen, tquery, tindex, _tiles_meta(d_meta)

    def poll(self):
        """utree_classify_poll: raises UtreeError(E_DEVICE) if a batch that has finished since the last call found its workspace
        too small (call after the stream has drained; its results are not to be used)."""
        _lib.check(_lib.load().utree_classify_poll(self._h), "utree_classify_poll")

    def rank_search(self, bases, off, length, rc: bool = False, slack: int = 2, sparsity: int = 4, tolerance: int = 2,
                    total_bases: Optional[int] = None, max_len: Optional[int] = None, out=None):
        """One batch of the rank-specific search (`xtree-search`, itree.c:969-1007).  Batches must come in file
        order: each read's vote also counts an entry left by an earlier read (itree.c:982); rank_reset() starts a
        new file.  Returns int32 [n, 6]: (mostIX, -2 printed / -4 not, hits kept, 0, most, secondMost)."""
        import torch
        n = off.numel()
        dev = bases.device
        if total_bases is None:
            total_bases = int(length.sum().item())
        if max_len is None:
            max_len = int(length.max().item()) if n else 0
        if out is None:
            out = torch.empty((n, 6), dtype=torch.int32, device=dev)
        prm = _lib.RankParams(slack, sparsity, tolerance)
        need = _lib.load().utree_rank_workspace_bytes(self._h, n, total_bases, max_len, int(rc), C.byref(prm))
        if n and not need:
            raise _lib.UtreeError(_lib.E_ARG, "utree_rank_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().utree_rank_batch(self._h, bases.data_ptr(), off.data_ptr(), length.data_ptr(), n,
                                                total_bases, max_len, int(rc), C.byref(prm), out.data_ptr(),
                                                self._ws.data_ptr(), self._ws.numel(), stream), "utree_rank_batch")
        return out

    def rank_reset(self):
        _lib.check(_lib.load().utree_rank_reset(self._h), "utree_rank_reset")

    def model_counts(self, bases, off, length, rc: bool = False) -> dict:
        """Measurement aid (bench.py's byte model): windows and distinct buckets / HBM lines per read of a batch."""
        import torch
        out = (C.c_uint64 * 5)()
        stream = torch.cuda.current_stream(bases.device).cuda_stream
        _lib.check(_lib.load().utree_model_counts(self._h, bases.data_ptr(), off.data_ptr(), length.data_ptr(), off.numel(), int(rc),
                                                  out, stream), "utree_model_counts")
        return dict(zip(("reads", "windows", "buckets", "lines128", "overflow_buckets"), [int(x) for x in out]))

    def kernel_name(self) -> str:
        return _lib.load().utree_classify_kernel_name(self._h).decode()

    def kernel_time(self, reset: bool = False):
        ms = C.c_double(0)
        n = C.c_uint64(0)
        _lib.check(_lib.load().utree_classify_kernel_time(self._h, int(reset), C.byref(ms), C.byref(n)),
                   "utree_classify_kernel_time")
        return ms.value, n.value

    def profile(self, capacity: int = 1 << 20) -> "Profile":
        """Per-taxon read counts on this device (utree_profile_create); `capacity` = slots for truncated taxa."""
        return Profile(self, capacity)

    def coverage(self, d_binix=None, d_records=None) -> "Coverage":
        """A coverage handle on this device (utree_coverage_create).  d_binix / d_records: torch uint8 CUDA tensors with the on-disk
        bin table and node dump (they are copied), or neither to stream the dump from the .ctr / the host copy."""
        return Coverage(self, d_binix, d_records)

    def redistribution(self, capacity: int = 1 << 22) -> "Redistribution":
        """A redistribution handle on this device (utree_redist_create); `capacity` = slots for distinct multi-label candidate sets."""
        return Redistribution(self, capacity)

    def samples(self, sample_capacity: int = 1 << 16, cell_capacity: int = 1 << 22, delim: bytes = b"_") -> "Samples":
        """A sample table on this device (utree_samples_create): at most sample_capacity distinct ids, cell_capacity (sample, taxon) slots."""
        return Samples(self, sample_capacity, cell_capacity, delim)

    def sample_redistribution(self, sample_capacity: int = 1 << 16, set_capacity: int = 1 << 22, cell_capacity: int = 1 << 22,
                              delim: bytes = b"_") -> "SampleRedistribution":
        """A per-sample redistribution handle on this device (utree_sredist_create): at most sample_capacity distinct ids, set_capacity slots
        for distinct multi-label candidate sets, cell_capacity (sample, candidate set) slots."""
        return SampleRedistribution(self, sample_capacity, set_capacity, cell_capacity, delim)

    def close(self):
        if self._h:
            _lib.load().utree_dev_free(self._h)
            self._h = None
            self._keep = None
            self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Profile:
    """Per-taxon read counts on one device (utree_profile_*): add() batches of classify / rank_search results, entries() reads
    them back, write() merges entries by their text and writes the profile file."""

    def __init__(self, tree: DeviceTree, capacity: int = 1 << 20):
        self.tree = tree
        h = C.c_void_p()
        _lib.check(_lib.load().utree_profile_create(tree._h, capacity, C.byref(h)), "utree_profile_create")
        self._h = h

    def add(self, results, n: Optional[int] = None):
        """results: the int32 [n, 6] CUDA tensor of classify() / rank_search(); asynchronous on torch's current stream."""
        import torch
        if not (isinstance(results, torch.Tensor) and results.dtype == torch.int32 and results.dim() == 2 and results.shape[1] == 6
                and results.is_contiguous() and results.is_cuda and results.device.index == self.tree.info.device):
            raise ValueError("Profile.add: results must be a contiguous int32 [n, 6] tensor on cuda:%d" % self.tree.info.device)
        n = results.shape[0] if n is None else n
        if not 0 <= n <= results.shape[0]:
            raise ValueError("Profile.add: n = %d outside the %d records given" % (n, results.shape[0]))
        stream = torch.cuda.current_stream(results.device).cuda_stream
        _lib.check(_lib.load().utree_profile_add(self._h, results.data_ptr(), n, stream), "utree_profile_add")

    def reset(self):
        _lib.check(_lib.load().utree_profile_reset(self._h), "utree_profile_reset")

    def entries(self):
        """(entries, n_reads, n_classified): entries a numpy array of PROFILE_ENTRY_DTYPE (label, cut, reads).  Raises
        UtreeError(E_DEVICE) when the table of truncated taxa was too small."""
        L = _lib.load()
        cap = L.utree_profile_max_entries(self._h)
        buf = np.zeros(cap, dtype=PROFILE_ENTRY_DTYPE)
        n = C.c_size_t(0)
        nr = C.c_uint64(0)
        nc = C.c_uint64(0)
        _lib.check(L.utree_profile_read(self._h, buf.ctypes.data, cap, C.byref(n), C.byref(nr), C.byref(nc)), "utree_profile_read")
        return buf[:n.value].copy(), nr.value, nc.value

    def write(self, path: str):
        e, nr, _ = self.entries()
        write_profile(self.tree.db, e, nr, path)

    def close(self):
        if self._h:
            _lib.load().utree_profile_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_profile(db: CtrDB, entries: np.ndarray, n_reads: int, path: str):
    """utree_profile_write: entries (PROFILE_ENTRY_DTYPE, from any number of devices) merged by text, rolled up, written."""
    e = np.ascontiguousarray(entries, dtype=PROFILE_ENTRY_DTYPE)
    _lib.check(_lib.load().utree_profile_write(db._h, e.ctypes.data if len(e) else None, len(e), n_reads, path.encode()),
               "utree_profile_write")


class SamplesReadback:
    """One handle's read-back (utree_samples_read): ids a list of bytes, reads / unclassified uint64 arrays per sample, cells a
    SAMPLES_CELL_DTYPE array, n_reads the records added.  Samples are numbered in the order the device first claimed their ids."""

    def __init__(self, ids, reads, unclassified, cells, n_reads):
        self.ids = list(ids)
        self.reads = np.ascontiguousarray(reads, dtype=np.uint64)
        self.unclassified = np.ascontiguousarray(unclassified, dtype=np.uint64)
        self.cells = np.ascontiguousarray(cells, dtype=SAMPLES_CELL_DTYPE)
        self.n_reads = int(n_reads)


class Samples:
    """Per-sample taxon table on one device (utree_samples_*): add() batches of records with their names, read() brings the ids, the
    per-sample counts and the (sample, label, cut) cells back, write() writes the table file."""

    def __init__(self, tree: DeviceTree, sample_capacity: int = 1 << 16, cell_capacity: int = 1 << 22, delim: bytes = b"_"):
        if not (isinstance(delim, (bytes, bytearray)) and len(delim) == 1):
            raise ValueError("Samples: delim must be one byte")
        self.tree = tree
        h = C.c_void_p()
        _lib.check(_lib.load().utree_samples_create(tree._h, sample_capacity, cell_capacity, delim[0], C.byref(h)), "utree_samples_create")
        self._h = h

    def add(self, text, name_off, name_len, results, n: Optional[int] = None):
        """text: uint8 CUDA tensor; name_off / name_len: int32 CUDA tensors of offsets into text (taken as unsigned) and lengths; results:
        the int32 [n, 6] tensor of classify() / rank_search().  Asynchronous on torch's current stream."""
        import torch
        dev = self.tree.info.device
        ok = lambda t, dt: isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous() and t.is_cuda and t.device.index == dev
        if not (ok(text, torch.uint8) and ok(name_off, torch.int32) and ok(name_len, torch.int32) and ok(results, torch.int32)
                and results.dim() == 2 and results.shape[1] == 6):
            raise ValueError("Samples.add: text uint8, name_off / name_len int32, results int32 [n, 6], all contiguous on cuda:%d" % dev)
        n = results.shape[0] if n is None else n
        if not (0 <= n <= results.shape[0] and n <= name_off.numel() and n <= name_len.numel()):
            raise ValueError("Samples.add: n = %d outside the records or names given" % n)
        stream = torch.cuda.current_stream(results.device).cuda_stream
        _lib.check(_lib.load().utree_samples_add(self._h, text.data_ptr(), text.numel(), name_off.data_ptr(), name_len.data_ptr(),
                                                 results.data_ptr(), n, stream), "utree_samples_add")

    def reset(self):
        _lib.check(_lib.load().utree_samples_reset(self._h), "utree_samples_reset")

    def read(self) -> SamplesReadback:
        """Raises UtreeError(E_DEVICE) when a table was too small or a record or name was refused: there is no table then."""
        L = _lib.load()
        ns, nb, nc, nr = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        code = L.utree_samples_read(self._h, None, 0, None, None, None, 0, None, 0, C.byref(ns), C.byref(nb), C.byref(nc), C.byref(nr))
        if code not in (_lib.OK, _lib.E_ARG):
            _lib.check(code, "utree_samples_read")
        S = ns.value
        ids = np.zeros(max(nb.value, 1), dtype=np.uint8)
        off = np.zeros(S + 1, dtype=np.uint64)
        reads = np.zeros(max(S, 1), dtype=np.uint64)
        uncl = np.zeros(max(S, 1), dtype=np.uint64)
        cells = np.zeros(max(nc.value, 1), dtype=SAMPLES_CELL_DTYPE)
        _lib.check(L.utree_samples_read(self._h, ids.ctypes.data, nb.value, off.ctypes.data, reads.ctypes.data, uncl.ctypes.data, S,
                                        cells.ctypes.data, nc.value, C.byref(ns), C.byref(nb), C.byref(nc), C.byref(nr)), "utree_samples_read")
        raw = ids.tobytes()
        return SamplesReadback([raw[int(off[i]):int(off[i + 1])] for i in range(S)], reads[:S], uncl[:S], cells[:nc.value].copy(), nr.value)

    def write(self, path: str):
        write_samples(self.tree.db, [self.read()], path)

    def close(self):
        if self._h:
            _lib.load().utree_samples_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_samples(db: CtrDB, readbacks: Sequence[SamplesReadback], path: str):
    """utree_samples_write: the read-backs of any number of handles, samples merged by id text and taxa by printed text, written."""
    tabs = (_lib.SamplesTable * max(len(readbacks), 1))()
    keep = []
    for t, rb in zip(tabs, readbacks):
        ids = np.frombuffer(b"".join(rb.ids) + b"\0", dtype=np.uint8).copy()
        off = np.zeros(len(rb.ids) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(i) for i in rb.ids], dtype=np.uint64) if rb.ids else []
        keep.append((ids, off, rb.reads, rb.unclassified, rb.cells))
        t.ids = ids.ctypes.data; t.id_off = off.ctypes.data
        t.reads = rb.reads.ctypes.data if len(rb.ids) else None
        t.unclassified = rb.unclassified.ctypes.data if len(rb.ids) else None
        t.n_samples = len(rb.ids)
        t.cells = rb.cells.ctypes.data if len(rb.cells) else None
        t.n_cells = len(rb.cells); t.n_reads = rb.n_reads
    _lib.check(_lib.load().utree_samples_write(db._h, tabs, len(readbacks), path.encode()), "utree_samples_write")


class Coverage:
    """Which database k-mers a sample touched, on one device (utree_coverage_*): add() batches of reads as classify() takes them,
    entries() reads back one (label, db_kmers, covered, hits) entry per label, write() writes the coverage file."""

    def __init__(self, tree: DeviceTree, d_binix=None, d_records=None):
        if (d_binix is None) != (d_records is None):
            raise ValueError("Coverage: give both d_binix and d_records, or neither")
        self.tree = tree
        h = C.c_void_p()
        _lib.check(_lib.load().utree_coverage_create(tree.db._h, tree._h, d_binix.data_ptr() if d_binix is not None else None,
                                                     d_records.data_ptr() if d_records is not None else None, C.byref(h)),
                   "utree_coverage_create")
        self._h = h

    @staticmethod
    def bytes_needed(db: CtrDB) -> int:
        return _lib.load().utree_coverage_bytes(db._h)

    def add(self, bases, off, length, rc: bool = False):
        """bases: uint8 CUDA tensor; off: int64; length: int32 (as DeviceTree.classify).  Asynchronous on torch's current stream."""
        import torch
        dev = self.tree.info.device
        for t, dt in ((bases, torch.uint8), (off, torch.int64), (length, torch.int32)):
            if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous() and t.is_cuda and t.device.index == dev):
                raise ValueError("Coverage.add: bases / off / length must be contiguous uint8 / int64 / int32 tensors on cuda:%d" % dev)
        if off.numel() != length.numel():
            raise ValueError("Coverage.add: %d offsets, %d lengths" % (off.numel(), length.numel()))
        stream = torch.cuda.current_stream(bases.device).cuda_stream
        _lib.check(_lib.load().utree_coverage_add(self._h, bases.data_ptr(), off.data_ptr(), length.data_ptr(), off.numel(), int(rc),
                                                  stream), "utree_coverage_add")

    def reset(self):
        _lib.check(_lib.load().utree_coverage_reset(self._h), "utree_coverage_reset")

    def merge(self, other: "Coverage"):
        """self += other (bitmaps OR-ed, counters added); the handles may be on different devices."""
        _lib.check(_lib.load().utree_coverage_merge(self._h, other._h), "utree_coverage_merge")

    def entries(self):
        """(entries, n_reads, n_hits): entries a numpy array of COVERAGE_ENTRY_DTYPE, one per label in index order."""
        L = _lib.load()
        cap = self.tree.db.info.n_labels
        buf = np.zeros(cap, dtype=COVERAGE_ENTRY_DTYPE)
        n = C.c_size_t(0)
        nr = C.c_uint64(0)
        nh = C.c_uint64(0)
        _lib.check(L.utree_coverage_read(self._h, buf.ctypes.data if cap else None, cap, C.byref(n), C.byref(nr), C.byref(nh)),
                   "utree_coverage_read")
        return buf[:n.value].copy(), nr.value, nh.value

    def write(self, path: str):
        e, nr, _ = self.entries()
        write_coverage(self.tree.db, e, nr, path)

    def close(self):
        if self._h:
            _lib.load().utree_coverage_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Redistribution:
    """Candidate sets of ambiguous reads on one device and their redistribution (utree_redist_*): classify() is DeviceTree.classify()
    that also adds the batch's sets, sets() reads every distinct set back, solve() runs the passes, write() writes the file."""

    def __init__(self, tree: DeviceTree, capacity: int = 1 << 22):
        self.tree = tree
        self._ws = None
        h = C.c_void_p()
        _lib.check(_lib.load().utree_redist_create(tree._h, capacity, C.byref(h)), "utree_redist_create")
        self._h = h

    def classify(self, bases, off, length, rc: bool = False, total_bases: Optional[int] = None, max_len: Optional[int] = None, out=None,
                 workspace=None, keys=None):
        """As DeviceTree.classify (the same results, bit for bit); the candidate sets of the batch are added on the way.  Asynchronous on
        torch's current stream; any number of streams may add at once (give each its own workspace).  keys: an int32 / uint32 tensor of one
        element per read on the reads' device -- every read's key goes there (utree_redist_classify_batch_keys), for assign()."""
        import torch
        n = off.numel()
        dev = bases.device
        if total_bases is None:
            total_bases = int(length.sum().item())
        if max_len is None:
            max_len = int(length.max().item()) if n else 0
        if out is None:
            out = torch.empty((n, 6), dtype=torch.int32, device=dev)
        need = self.tree.workspace_bytes(n, total_bases, max_len, rc)
        if workspace is None:
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = self._ws
        stream = torch.cuda.current_stream(dev).cuda_stream
        if keys is not None:
            if keys.numel() != n or keys.element_size() != 4 or not keys.is_contiguous() or keys.device != dev:
                raise ValueError("Redistribution.classify: keys must be a contiguous 4-byte tensor of one element per read on the reads' device")
            _lib.check(_lib.load().utree_redist_classify_batch_keys(self._h, self.tree._h, bases.data_ptr(), off.data_ptr(), length.data_ptr(), n,
                                                                    total_bases, max_len, int(rc), out.data_ptr(), workspace.data_ptr(),
                                                                    workspace.numel(), keys.data_ptr(), stream), "utree_redist_classify_batch_keys")
            return out
        _lib.check(_lib.load().utree_redist_classify_batch(self._h, self.tree._h, bases.data_ptr(), off.data_ptr(), length.data_ptr(), n,
                                                           total_bases, max_len, int(rc), out.data_ptr(), workspace.data_ptr(),
                                                           workspace.numel(), stream), "utree_redist_classify_batch")
        return out

    def assign(self, keys, solved: Optional["Redistribution"] = None):
        """(label, ncand): int32 tensors (bit patterns of uint32) of one element per key -- the label the last solve() of `solved` (this handle,
        or the one this handle was merged into) assigns each read to, and how many candidates the read had; 0xFFFFFFFF and 0 for a read
        without a hit (utree_redist_assign).  keys: what classify(keys=) of THIS handle wrote.  Asynchronous on torch's current stream once
        the slots' winners stand (once per solve)."""
        import torch
        if keys.element_size() != 4 or not keys.is_contiguous():
            raise ValueError("Redistribution.assign: keys must be a contiguous 4-byte tensor")
        n = keys.numel()
        label = torch.empty(n, dtype=torch.int32, device=keys.device)
        ncand = torch.empty(n, dtype=torch.int32, device=keys.device)
        stream = torch.cuda.current_stream(keys.device).cuda_stream
        _lib.check(_lib.load().utree_redist_assign(self._h, (solved or self)._h, keys.data_ptr() if n else None, n, label.data_ptr() if n else None,
                                                   ncand.data_ptr() if n else None, stream), "utree_redist_assign")
        return label, ncand

    def sets(self):
        """(sets, n_reads, n_classified): sets = {sorted tuple of file-order label indices: reads}, single-label sets included.  Raises
        UtreeError(E_DEVICE) when the table or the arena was too small."""
        L = _lib.load()
        ns, nl, nr, nc = C.c_size_t(0), C.c_size_t(0), C.c_uint64(0), C.c_uint64(0)
        code = L.utree_redist_read(self._h, None, 0, None, 0, C.byref(ns), C.byref(nl), C.byref(nr), C.byref(nc))
        if code not in (_lib.OK, _lib.E_ARG):
            _lib.check(code, "utree_redist_read")
        s = np.zeros(max(ns.value, 1), dtype=REDIST_SET_DTYPE)
        lab = np.zeros(max(nl.value, 1), dtype=np.uint32)
        _lib.check(L.utree_redist_read(self._h, s.ctypes.data, ns.value, lab.ctypes.data, nl.value, C.byref(ns), C.byref(nl), C.byref(nr),
                                       C.byref(nc)), "utree_redist_read")
        out = {}
        for reads, first, n, _ in s[:ns.value].tolist():
            key = tuple(sorted(lab[first:first + n].tolist()))
            out[key] = out.get(key, 0) + reads
        return out, nr.value, nc.value

    def merge(self, other: "Redistribution"):
        """self += other (sets re-inserted, counters added); the handles may be on different devices."""
        _lib.check(_lib.load().utree_redist_merge(self._h, other._h), "utree_redist_merge")

    def solve(self, max_passes: int = 100):
        """(entries, passes, ambiguous): entries a numpy array of REDIST_ENTRY_DTYPE (label, assigned, unique), labels with a figure only."""
        cap = self.tree.db.info.n_labels
        buf = np.zeros(max(cap, 1), dtype=REDIST_ENTRY_DTYPE)
        n, p, a = C.c_size_t(0), C.c_uint32(0), C.c_uint64(0)
        _lib.check(_lib.load().utree_redist_solve(self._h, max_passes, buf.ctypes.data, cap, C.byref(n), C.byref(p), C.byref(a)),
                   "utree_redist_solve")
        return buf[:n.value].copy(), p.value, a.value

    def write(self, path: str, max_passes: int = 100):
        e, p, a = self.solve(max_passes)
        _, nr, _ = self.sets()
        write_redistribution(self.tree.db, e, nr, a, p, path)

    def reset(self):
        _lib.check(_lib.load().utree_redist_reset(self._h), "utree_redist_reset")

    def close(self):
        if self._h:
            _lib.load().utree_redist_free(self._h)
            self._h = None
            self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SredistReadback:
    """One handle's read-back (utree_sredist_read): ids a list of bytes, reads / unclassified uint64 arrays per sample, cells a
    SREDIST_CELL_DTYPE array into the flat uint32 array labels, n_reads the records added."""

    def __init__(self, ids, reads, unclassified, cells, labels, n_reads):
        self.ids = list(ids)
        self.reads = np.ascontiguousarray(reads, dtype=np.uint64)
        self.unclassified = np.ascontiguousarray(unclassified, dtype=np.uint64)
        self.cells = np.ascontiguousarray(cells, dtype=SREDIST_CELL_DTYPE)
        self.labels = np.ascontiguousarray(labels, dtype=np.uint32)
        self.n_reads = int(n_reads)

    def multisets(self):
        """{sample id: {sorted tuple of file-order label indices: reads}}, every sample of the read-back a key"""
        out = {i: {} for i in self.ids}
        for s, n, first, reads in self.cells.tolist():
            key = tuple(sorted(self.labels[first:first + n].tolist()))
            d = out[self.ids[s]]
            d[key] = d.get(key, 0) + reads
        return out


def _ids_flat(ids):
    raw = np.frombuffer(b"".join(ids) + b"\0", dtype=np.uint8).copy()
    off = np.zeros(len(ids) + 1, dtype=np.uint64)
    if ids:
        off[1:] = np.cumsum([len(i) for i in ids], dtype=np.uint64)
    return raw, off


class SampleRedistribution:
    """Candidate sets per sample on one device and every sample's redistribution (utree_sredist_*): classify() is DeviceTree.classify()
    that also counts the batch's reads per (sample, candidate set), read() brings ids, counts and cells back, insert() adds such a read-back,
    solve() runs every sample's passes, write() writes the file."""

    def __init__(self, tree: DeviceTree, sample_capacity: int = 1 << 16, set_capacity: int = 1 << 22, cell_capacity: int = 1 << 22,
                 delim: bytes = b"_"):
        if not (isinstance(delim, (bytes, bytearray)) and len(delim) == 1):
            raise ValueError("SampleRedistribution: delim must be one byte")
        self.tree = tree
        self._ws = None
        h = C.c_void_p()
        _lib.check(_lib.load().utree_sredist_create(tree._h, sample_capacity, set_capacity, cell_capacity, delim[0], C.byref(h)),
                   "utree_sredist_create")
        self._h = h

    def classify(self, bases, off, length, text, name_off, name_len, rc: bool = False, total_bases: Optional[int] = None,
                 max_len: Optional[int] = None, out=None, workspace=None):
        """As DeviceTree.classify (the same results, bit for bit) with the reads' names as Samples.add takes them: text uint8, name_off /
        name_len int32 CUDA tensors.  Asynchronous on torch's current stream; any number of streams may add at once (give each its own
        workspace)."""
        import torch
        n = off.numel()
        dev = bases.device
        ok = lambda t, dt: isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous() and t.is_cuda and t.device == dev
        if not (ok(text, torch.uint8) and ok(name_off, torch.int32) and ok(name_len, torch.int32) and name_off.numel() >= n and name_len.numel() >= n):
            raise ValueError("SampleRedistribution.classify: text uint8, name_off / name_len int32 with a name per read, contiguous on the reads' device")
        if total_bases is None:
            total_bases = int(length.sum().item())
        if max_len is None:
            max_len = int(length.max().item()) if n else 0
        if out is None:
            out = torch.empty((n, 6), dtype=torch.int32, device=dev)
        need = self.tree.workspace_bytes(n, total_bases, max_len, rc)
        if workspace is None:
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = self._ws
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().utree_sredist_classify_batch(self._h, self.tree._h, bases.data_ptr(), off.data_ptr(), length.data_ptr(), n,
                                                            total_bases, max_len, int(rc), text.data_ptr(), text.numel(), name_off.data_ptr(),
                                                            name_len.data_ptr(), out.data_ptr(), workspace.data_ptr(), workspace.numel(), stream),
                   "utree_sredist_classify_batch")
        return out

    def read(self) -> SredistReadback:
        """Raises UtreeError(E_DEVICE) when a table was too small or a record or name was refused: there is no table then."""
        L = _lib.load()
        ns, nb, nc, nl, nr = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        code = L.utree_sredist_read(self._h, None, 0, None, None, None, 0, None, 0, None, 0, C.byref(ns), C.byref(nb), C.byref(nc), C.byref(nl),
                                    C.byref(nr))
        if code not in (_lib.OK, _lib.E_ARG):
            _lib.check(code, "utree_sredist_read")
        S = ns.value
        ids = np.zeros(max(nb.value, 1), dtype=np.uint8)
        off = np.zeros(S + 1, dtype=np.uint64)
        reads = np.zeros(max(S, 1), dtype=np.uint64)
        uncl = np.zeros(max(S, 1), dtype=np.uint64)
        cells = np.zeros(max(nc.value, 1), dtype=SREDIST_CELL_DTYPE)
        labels = np.zeros(max(nl.value, 1), dtype=np.uint32)
        _lib.check(L.utree_sredist_read(self._h, ids.ctypes.data, nb.value, off.ctypes.data, reads.ctypes.data, uncl.ctypes.data, S,
                                        cells.ctypes.data, nc.value, labels.ctypes.data, nl.value, C.byref(ns), C.byref(nb), C.byref(nc),
                                        C.byref(nl), C.byref(nr)), "utree_sredist_read")
        raw = ids.tobytes()
        return SredistReadback([raw[int(off[i]):int(off[i + 1])] for i in range(S)], reads[:S], uncl[:S], cells[:nc.value].copy(),
                               labels[:nl.value].copy(), nr.value)

    def insert(self, rb: SredistReadback):
        """utree_sredist_insert: the ids, counts and cells of a read-back (or of the same form made on the host) added to this handle."""
        raw, off = _ids_flat(rb.ids)
        S = len(rb.ids)
        _lib.check(_lib.load().utree_sredist_insert(self._h, raw.ctypes.data, off.ctypes.data, rb.reads.ctypes.data if S else None,
                                                    rb.unclassified.ctypes.data if S else None, S, rb.cells.ctypes.data if len(rb.cells) else None,
                                                    len(rb.cells), rb.labels.ctypes.data if len(rb.labels) else None, len(rb.labels), rb.n_reads),
                   "utree_sredist_insert")

    def merge(self, other: "SampleRedistribution"):
        """self += other; the handles may be on different devices."""
        _lib.check(_lib.load().utree_sredist_merge(self._h, other._h), "utree_sredist_merge")

    def solve(self, max_passes: int = 100, n_samples: Optional[int] = None, n_labels: Optional[int] = None):
        """(entries, passes, ambiguous): entries a SREDIST_ENTRY_DTYPE array ((sample, label) with a figure only, samples numbered as read()
        numbers them), passes and ambiguous arrays per sample."""
        if n_samples is None or n_labels is None:
            rb = self.read()
            n_samples, n_labels = len(rb.ids), len(rb.labels)
        buf = np.zeros(max(n_labels, 1), dtype=SREDIST_ENTRY_DTYPE)
        p = np.zeros(max(n_samples, 1), dtype=np.uint32)
        a = np.zeros(max(n_samples, 1), dtype=np.uint64)
        n, s = C.c_size_t(0), C.c_size_t(0)
        _lib.check(_lib.load().utree_sredist_solve(self._h, max_passes, buf.ctypes.data, n_labels, C.byref(n), p.ctypes.data, a.ctypes.data,
                                                   n_samples, C.byref(s)), "utree_sredist_solve")
        return buf[:n.value].copy(), p[:s.value].copy(), a[:s.value].copy()

    def write(self, path: str, max_passes: int = 100):
        rb = self.read()
        e, p, a = self.solve(max_passes, len(rb.ids), len(rb.labels))
        write_sample_redistribution(self.tree.db, rb.ids, rb.reads, rb.unclassified, p, a, e, rb.n_reads, path)

    def reset(self):
        _lib.check(_lib.load().utree_sredist_reset(self._h), "utree_sredist_reset")

    def close(self):
        if self._h:
            _lib.load().utree_sredist_free(self._h)
            self._h = None
            self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_sample_redistribution(db: CtrDB, ids, reads, unclassified, passes, ambiguous, entries, n_reads: int, path: str):
    """utree_sredist_write (host only): the samples of a read-back and the figures of a solve, labels merged by text, written."""
    raw, off = _ids_flat(list(ids))
    S = len(ids)
    r, u = np.ascontiguousarray(reads, dtype=np.uint64), np.ascontiguousarray(unclassified, dtype=np.uint64)
    p, a = np.ascontiguousarray(passes, dtype=np.uint32), np.ascontiguousarray(ambiguous, dtype=np.uint64)
    if not (len(r) == len(u) == len(p) == len(a) == S):
        raise ValueError("write_sample_redistribution: one figure per sample")
    e = np.ascontiguousarray(entries, dtype=SREDIST_ENTRY_DTYPE)
    _lib.check(_lib.load().utree_sredist_write(db._h, raw.ctypes.data, off.ctypes.data, r.ctypes.data if S else None, u.ctypes.data if S else None,
                                               p.ctypes.data if S else None, a.ctypes.data if S else None, S, e.ctypes.data if len(e) else None,
                                               len(e), n_reads, path.encode()), "utree_sredist_write")


def write_redistribution(db: CtrDB, entries: np.ndarray, n_reads: int, ambiguous: int, passes: int, path: str):
    """utree_redist_write: entries (REDIST_ENTRY_DTYPE, from any number of solves) merged by text, rolled up, written."""
    e = np.ascontiguousarray(entries, dtype=REDIST_ENTRY_DTYPE)
    _lib.check(_lib.load().utree_redist_write(db._h, e.ctypes.data if len(e) else None, len(e), n_reads, ambiguous, passes, path.encode()),
               "utree_redist_write")


def write_coverage(db: CtrDB, entries: np.ndarray, n_reads: int, path: str):
    """utree_coverage_write: entries (COVERAGE_ENTRY_DTYPE; all labels of the database) merged by text, rolled up, written."""
    e = np.ascontiguousarray(entries, dtype=COVERAGE_ENTRY_DTYPE)
    _lib.check(_lib.load().utree_coverage_write(db._h, e.ctypes.data if len(e) else None, len(e), n_reads, path.encode()),
               "utree_coverage_write")


def search_gg(db: CtrDB, trees: Sequence[DeviceTree], fasta: str, out: str, rc: bool = False, threads: int = 0,
              input_format: int = _lib.INPUT_REFERENCE, profile: Optional[str] = None, coverage: Optional[str] = None,
              mates: Optional[str] = None, interleaved: bool = False, redistribute: Optional[str] = None, redist_passes: int = 100,
              hitmap: Optional[str] = None, samples: Optional[str] = None, sample_delim: bytes = b"_",
              sample_redistribute: Optional[str] = None, redistribute_reads: Optional[str] = None):
    """XT_doSearch32(utree, in, out, 8, speed, doRC) (itree.c:833) as one utree_search_request through utree_search_run (the utree_search_file*
    calls named below are its fixed-argument forms): returns (code, stats); stats.fasta_error says which of
    the reference's exit(2) conditions a malformed read hit.  input_format != INPUT_REFERENCE opts into FASTQ / multi-line
    FASTA / gzip input.  profile: also write the per-taxon read counts there; coverage: also write the per-taxon k-mer
    coverage there (utree_search_file_coverage; None: no such report).
    Paired-end reads (utree_search_pairs_file): mates = the file of second mates, or interleaved=True when `fasta` holds records 2i and
    2i+1 of pair i.  A pair is searched as mate 1 + "N" + mate 2, named by mate 1 (mate names are not compared); stats.n_reads counts
    pairs; unequal record counts return E_PAIRS after the complete pairs were written.
    redistribute: also write the reads redistributed among the labels each hit most often there (utree_search_file_redistribute), at most
    redist_passes passes; a redistribution that cannot be written returns E_PROFILE.
    hitmap: also write every query's k-mer hit map there, and the label texts to hitmap + ".labels" (utree_search_file_hitmap); a map that
    cannot be written returns E_HITMAP.
    samples: the reads are a combined file named <sample><sample_delim><n>; also write the taxon x sample table there
    (utree_search_file_samples); a table that cannot be written returns E_PROFILE.
    sample_redistribute: also write the taxon x sample table with every sample's ambiguous reads redistributed within that sample there
    (utree_search_file_sample_redistribute; ids cut at sample_delim, at most redist_passes passes per sample); E_PROFILE likewise.
    redistribute_reads: also write, for every query with a line in `out` and in that order, "name\\tlabel text\\tn_candidates" there -- the label
    the redistribution assigns the read to (with or without redistribute=: one solve serves both); host framing pipeline; E_PROFILE likewise."""
    if mates is not None and interleaved:
        raise ValueError("search_gg: give mates= or interleaved=True, not both")
    arr = (C.c_void_p * len(trees))(*[t._h for t in trees])
    return _search_run(db, arr, len(trees), "search_gg", fasta, out, rc, threads, input_format, sample_delim, mates_path=mates, interleaved=int(interleaved),
                       profile_path=profile, coverage_path=coverage, redistribute_path=redistribute, max_passes=redist_passes, hitmap_path=hitmap,
                       samples_path=samples, sample_redistribute_path=sample_redistribute, redistribute_reads_path=redistribute_reads)


def _search_run(db, arr, n_dev, who, fasta, out, rc, threads, input_format, sample_delim, **fields):
    """One SearchRequest from search_gg's / search_rank's arguments (paths: str or None), one utree_search_run: (code, stats)."""
    req = _lib.SearchRequest(do_rc=int(rc), host_threads=threads, input_format=input_format, reads_path=fasta.encode(), out_path=out.encode())
    for k, v in fields.items():
        setattr(req, k, v.encode() if isinstance(v, str) else v)
    if req.samples_path is not None or req.sample_redistribute_path is not None:
        if not (isinstance(sample_delim, (bytes, bytearray)) and len(sample_delim) == 1):
            raise ValueError("%s: sample_delim must be one byte" % who)
        req.sample_delim = sample_delim[0]
    st = _lib.SearchStats()
    code = _lib.load().utree_search_run(db._h, arr, n_dev, C.byref(req), C.byref(st))
    return code, st


def search_rank(db: CtrDB, tree: DeviceTree, fasta: str, out: str, rc: bool = False, slack: int = 2, sparsity: int = 4,
                tolerance: int = 2, threads: int = 0, input_format: int = _lib.INPUT_REFERENCE, profile: Optional[str] = None,
                samples: Optional[str] = None, sample_delim: bytes = b"_"):
    """XT_doSearch32(utree, in, out, 0, speed, doRC): the `xtree-search` binary (itree.c:1376 without DO_GG).  profile, samples,
    sample_delim: as search_gg's."""
    prm = _lib.RankParams(slack, sparsity, tolerance)
    return _search_run(db, (C.c_void_p * 1)(tree._h), 1, "search_rank", fasta, out, rc, threads, input_format, sample_delim, rank=C.pointer(prm),
                       profile_path=profile, samples_path=samples)


def build(fasta: str, mapfile: str, ubt: str, W: int = 8, I: int = 2, complevel: int = 1, gg: bool = True, device: int = 0):
    """`utree-build[GG] in.fa labels.map out.ubt threads complevel` (itree.c:1379-1407): returns (code, stats)."""
    st = _lib.BuildStats()
    code = _lib.load().utree_build_file(fasta.encode(), mapfile.encode(), ubt.encode(), W, I, complevel, int(gg), device,
                                        C.byref(st))
    return code, st


def compress(ubt: str, ctr: str, device: int = 0):
    """XT_cmp32(preTree.ubt, compTree.ctr) (itree.c:1234): returns (code, stats)."""
    st = _lib.CompressStats()
    code = _lib.load().utree_compress_file(ubt.encode(), ctr.encode(), device, C.byref(st))
    return code, st


def merge(inputs, ubt: str, gg: bool = True, I: int = 0, device: int = 0):
    """`utree-merge[GG] out.ubt in1 [in2 ...]`: the `.ubt` / `.ctr` databases `inputs` folded into one `.ubt` as the builder's insert loop
    would (include/utree_amd.h: utree_merge_files).  Returns the MergeStats; raises UtreeError (with .detail: what utree_last_hip_error
    said) when the call fails, and no output file is left then."""
    paths = [p.encode() for p in inputs]
    arr = (C.c_char_p * max(len(paths), 1))(*paths)
    st = _lib.MergeStats()
    L = _lib.load()
    code = L.utree_merge_files(arr, len(paths), ubt.encode(), I, int(gg), device, C.byref(st))
    if code != _lib.OK:
        detail = (L.utree_last_hip_error() or b"").decode(errors="replace")
        e = _lib.UtreeError(code, "merge: " + detail)
        e.detail = detail
        e.stats = st
        raise e
    return st


def _merge_edit_struct(ranks, drop, keep, rename, minus):
    """(the MergeEdit, what must stay alive while it is in use)"""
    mp = [p.encode() for p in minus]
    arr = (C.c_char_p * max(len(mp), 1))(*mp)
    enc = lambda p: p.encode() if p is not None else None
    ed = _lib.MergeEdit(ranks=ranks, drop_path=enc(drop), keep_path=enc(keep), rename_path=enc(rename),
                        minus_paths=C.cast(arr, C.POINTER(C.c_char_p)) if mp else None, n_minus=len(mp))
    return ed, arr


def merge_edit(inputs, ubt: str, gg: bool = True, I: int = 0, device: int = 0, ranks: int = 0, drop=None, keep=None, rename=None, minus=()):
    """merge() with an edit (include/utree_amd.h: utree_merge_files_edit): labels cut to their first `ranks` ranks, the clades listed in the
    file `drop` dropped, only those in `keep` kept, clades renamed by the `old TAB new` lines of `rename`, and every word that a database
    of `minus` holds subtracted.  Returns (MergeStats, MergeEditStats); raises UtreeError as merge() does (.edit_stats is set too)."""
    paths = [p.encode() for p in inputs]
    arr = (C.c_char_p * max(len(paths), 1))(*paths)
    ed, _alive = _merge_edit_struct(ranks, drop, keep, rename, minus)
    st, es = _lib.MergeStats(), _lib.MergeEditStats()
    L = _lib.load()
    code = L.utree_merge_files_edit(arr, len(paths), ubt.encode(), I, int(gg), device, C.byref(ed), C.byref(st), C.byref(es))
    if code != _lib.OK:
        detail = (L.utree_last_hip_error() or b"").decode(errors="replace")
        e = _lib.UtreeError(code, "merge_edit: " + detail)
        e.detail = detail
        e.stats, e.edit_stats = st, es
        raise e
    return st, es


def merge_preview(inputs, tsv: str, ranks: int = 0, drop=None, keep=None, rename=None):
    """What merge_edit's label edit would do to every label line of `inputs`, written to `tsv` (host only, utree_merge_edit_preview).
    Returns the MergeEditStats; raises UtreeError, and no file is left then."""
    paths = [p.encode() for p in inputs]
    arr = (C.c_char_p * max(len(paths), 1))(*paths)
    ed, _alive = _merge_edit_struct(ranks, drop, keep, rename, ())
    es = _lib.MergeEditStats()
    L = _lib.load()
    code = L.utree_merge_edit_preview(arr, len(paths), C.byref(ed), tsv.encode(), C.byref(es))
    if code != _lib.OK:
        detail = (L.utree_last_hip_error() or b"").decode(errors="replace")
        e = _lib.UtreeError(code, "merge_preview: " + detail)
        e.detail = detail
        raise e
    return es


def merge_probe(path: str):
    """How utree_merge_files reads one input (host only): the MergeInput (W, I, is_ctr, n_nodes, n_labels); raises UtreeError."""
    info = _lib.MergeInput()
    L = _lib.load()
    code = L.utree_merge_probe(path.encode(), C.byref(info))
    if code != _lib.OK:
        detail = (L.utree_last_hip_error() or b"").decode(errors="replace")
        e = _lib.UtreeError(code, "merge_probe: " + detail)
        e.detail = detail
        raise e
    return info


def compare(a: str, b: str, report: str, moves=None, device: int = 0):
    """`utree-compare old new report.tsv [moves.tsv]`: the `.ubt` / `.ctr` database `a` ("old") against `b` ("new"), word by word and label
    text by label text (include/utree_amd.h: utree_compare_files).  `report` gets the per-taxon figures, `moves` (or None) the distinct
    (label in a, label in b) pairs of the words whose label changed.  Returns the CompareStats; raises UtreeError (with .detail: what
    utree_last_hip_error said) when the call fails, and neither file is left then."""
    st = _lib.CompareStats()
    L = _lib.load()
    code = L.utree_compare_files(a.encode(), b.encode(), report.encode(), moves.encode() if moves is not None else None, device, C.byref(st))
    if code != _lib.OK:
        detail = (L.utree_last_hip_error() or b"").decode(errors="replace")
        e = _lib.UtreeError(code, "compare: " + detail)
        e.detail = detail
        e.stats = st
        raise e
    return st


def inspect(db: str, report: str, pairs=None, device: int = 0):
    """`utree-inspect db report.tsv [pairs.tsv]`: which k-mers of the `.ubt` / `.ctr` database `db` have a neighbour one substitution away,
    and under which label (include/utree_amd.h: utree_inspect_file).  `report` gets the per-taxon classes, `pairs` (or None) the distinct
    ordered pairs of label texts one substitution apart.  Returns the InspectStats; raises UtreeError (with .detail: what
    utree_last_hip_error said) when the call fails, and neither file is left then."""
    st = _lib.InspectStats()
    L = _lib.load()
    code = L.utree_inspect_file(db.encode(), report.encode(), pairs.encode() if pairs is not None else None, device, C.byref(st))
    if code != _lib.OK:
        detail = (L.utree_last_hip_error() or b"").decode(errors="replace")
        e = _lib.UtreeError(code, "inspect: " + detail)
        e.detail = detail
        e.stats = st
        raise e
    return st


def _tiles_meta(d_meta):
    m = _lib.TilesMeta.from_buffer_copy(d_meta.cpu().numpy().tobytes())
    return dict(total_tiles=int(m.total_tiles), total_bases=int(m.total_bases), max_len=int(m.max_len), error=int(m.error))


def _tiles_text(what, cap, call):
    bad = C.c_size_t(-1).value
    while True:
        out = np.empty(cap, dtype=np.uint8)
        n = call(out)
        if n != bad:
            return out[:n].tobytes()
        if cap > (1 << 34):
            raise _lib.UtreeError(_lib.E_NOMEM, what)
        cap *= 4


def tiles_format(db: CtrDB, buf, name_off, name_len, seq_len, tile_bp: int, step_bp: int, tquery, tindex, results):
    """utree_tiles_format: the lines of tiles.tsv for tiles (tquery, tindex) of the framed queries and their results.  Returns (text, lines)."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    name_off, name_len = np.ascontiguousarray(name_off, dtype=np.uint64), np.ascontiguousarray(name_len, dtype=np.uint32)
    seq_len, tquery, tindex = (np.ascontiguousarray(a, dtype=np.uint32) for a in (seq_len, tquery, tindex))
    results = np.ascontiguousarray(results)
    assert (results.dtype.itemsize == 24 or results.dtype == np.int32) and results.nbytes == 24 * len(tquery) and len(tquery) == len(tindex)
    lines = C.c_uint64(0)

    def call(out):
        lines.value = 0
        return _lib.load().utree_tiles_format(db._h, buf.ctypes.data, name_off.ctypes.data, name_len.ctypes.data, seq_len.ctypes.data, tile_bp,
                                              step_bp, tquery.ctypes.data, tindex.ctypes.data, results.ctypes.data, len(tquery), out.ctypes.data,
                                              len(out), C.byref(lines))
    text = _tiles_text("utree_tiles_format", int(name_len.sum()) + 4096, call)
    return text, lines.value


def tiles_segments_format(db: CtrDB, buf, name_off, name_len, seq_len, tile_bp: int, step_bp: int, tquery, tindex, results, flush: bool = True,
                          state=None):
    """utree_tiles_segments_format: the lines of segments.tsv; `state` (a lib.TilesRun, or None for a fresh one) carries the open run from
    one call to the next, flush closes it.  Returns (text, lines)."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    name_off, name_len = np.ascontiguousarray(name_off, dtype=np.uint64), np.ascontiguousarray(name_len, dtype=np.uint32)
    seq_len, tquery, tindex = (np.ascontiguousarray(a, dtype=np.uint32) for a in (seq_len, tquery, tindex))
    results = np.ascontiguousarray(results)
    assert (results.dtype.itemsize == 24 or results.dtype == np.int32) and results.nbytes == 24 * len(tquery) and len(tquery) == len(tindex)
    if state is None:
        state = _lib.TilesRun()
    lines = C.c_uint64(0)

    def call(out):
        lines.value = 0
        return _lib.load().utree_tiles_segments_format(db._h, buf.ctypes.data, name_off.ctypes.data, name_len.ctypes.data, seq_len.ctypes.data,
                                                       tile_bp, step_bp, tquery.ctypes.data, tindex.ctypes.data, results.ctypes.data, len(tquery),
                                                       int(flush), C.byref(state), out.ctypes.data, len(out), C.byref(lines))
    text = _tiles_text("utree_tiles_segments_format", int(name_len.sum()) + 4096, call)
    return text, lines.value


def tiles_file(db: CtrDB, tree: DeviceTree, reads: str, tiles: str, segments=None, tile_bp: int = 1000, step_bp=None, rc: bool = False,
               input_format: int = _lib.INPUT_REFERENCE, threads: int = 0):
    """`utree-tiles db contigs.fa tiles.tsv [segments.tsv] [RC]`: every query of `reads` classified tile by tile (include/utree_amd.h:
    utree_tiles_file).  Returns (code, TilesStats): code is OK, or E_FASTA after a malformed record (the tiles of the queries in front of it
    are written); any other failure raises UtreeError, and neither file is left then."""
    if step_bp is None:
        step_bp = max(tile_bp // 2, 1)
    prm = _lib.TilesParams(tile_bp=tile_bp, step_bp=step_bp, do_rc=int(rc), input_format=input_format, host_threads=threads)
    st = _lib.TilesStats()
    code = _lib.load().utree_tiles_file(db._h, tree._h, reads.encode(), tiles.encode(), segments.encode() if segments is not None else None,
                                        C.byref(prm), C.byref(st))
    if code not in (_lib.OK, _lib.E_FASTA):
        raise _lib.UtreeError(code, "utree_tiles_file")
    return code, st


def classify_fasta_bytes(db: CtrDB, tree: DeviceTree, data: bytes, rc: bool = False) -> bytes:
    """Convenience for tests: frame -> upload -> classify -> format, through the C-ABI pieces."""
    import torch
    fr = frame_fasta(data, final=True)
    n = len(fr["seq_off"])
    dev = "cuda:%d" % tree.info.device
    if n == 0:
        return b""
    buf = np.frombuffer(data, dtype=np.uint8)
    d_buf = torch.from_numpy(buf.copy()).to(dev)
    d_off = torch.from_numpy(fr["seq_off"].astype(np.int64)).to(dev)
    d_len = torch.from_numpy(fr["seq_len"].astype(np.int32)).to(dev)
    res = tree.classify(d_buf, d_off, d_len, rc=rc, total_bases=int(fr["seq_len"].sum()),
                        max_len=int(fr["seq_len"].max()))
    torch.cuda.synchronize()
    tree.poll()
    h = res.cpu().numpy()
    return db.format(buf, fr["name_off"], fr["name_len"], h)
