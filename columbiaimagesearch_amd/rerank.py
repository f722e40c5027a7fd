"""Exact re-ranking of search results with the original features kept resident in HBM.

The reference fetches the features of the first ``rerank_nb`` results from HBase and replaces the ADC distance by the
true L2 distance (cufacesearch/cufacesearch/searcher/searcher_lopqhbase.py:864-912 and :975-1017):

    results = results[:min(rerank_nb, len(results))]
    dist    = np.linalg.norm(normed_feat - res_fts[pos])     # NOT squared; ADC distances are squared (:887,:998)
    (a result whose feature is missing keeps its ADC distance, :889-893)
    keep if not filter_near_dup or dist <= near_dup_th; only results with index < max_returned (index BEFORE the re-order)
    order = np.argsort(dists)

1M x 4096 float32 features are 16 GB: they fit the 288 GB of one MI355X, so the fetch becomes a gather in HBM.
"""
import numpy as np

from . import _lib


class ResidentFeatures(object):
    """Features [n, D] (float32 or float64 torch tensor on the GPU) + the ids of their rows."""

    def __init__(self, feats, ids=None):
        import torch
        if not (feats.is_cuda and feats.is_contiguous() and feats.dim() == 2 and feats.dtype in (torch.float32, torch.float64)):
            raise ValueError("feats must be a contiguous float32/float64 [n, D] tensor on the GPU")
        self.feats = feats
        self._ids = None if ids is None else list(ids)
        self._row = None if ids is None else {k: i for i, k in enumerate(self._ids)}
        self._dmap = None  # (keys, rows, event of the build): device_map

    def rows_of(self, ids):
        """Feature row of every id ([nq, L] array-like; -1 where the id is unknown or negative)."""
        ids = np.asarray(ids)
        if self._row is None:
            rows = ids.astype(np.int64).copy()
            rows[(rows < 0) | (rows >= self.feats.shape[0])] = -1
            return rows
        return np.array([[self._row.get(k.item() if hasattr(k, "item") else k, -1) for k in r] for r in ids], dtype=np.int64).reshape(ids.shape)

    def distances_dev(self, q, rows):
        """True L2 distances [nq, L] (float64 tensor; NaN where rows < 0) of queries q [nq, D] to feats[rows]."""
        import torch
        if not (q.is_cuda and q.is_contiguous() and q.dtype == self.feats.dtype and q.shape[1] == self.feats.shape[1]):
            raise ValueError("q must be a contiguous tensor on the GPU with the features' dtype and width")
        rows = rows if torch.is_tensor(rows) else torch.as_tensor(np.ascontiguousarray(rows, dtype=np.int64))
        rows = rows.to(q.device).contiguous()
        nq, L = int(rows.shape[0]), int(rows.shape[1])
        out = torch.empty((nq, L), dtype=torch.float64, device=q.device)
        code = _lib.CIS_F32 if q.dtype == torch.float32 else _lib.CIS_F64
        _lib.check(_lib.lib().cis_rerank_dev(self.feats.data_ptr(), code, int(self.feats.shape[0]), int(self.feats.shape[1]),
                                             q.data_ptr(), nq, rows.data_ptr(), L, out.data_ptr(),
                                             torch.cuda.current_stream(q.device).cuda_stream))
        return out

    def search_exact(self, q, k):
        """The exact k nearest resident features of every query (include/cis_hip.h:cis_exact_knn_dev): (ids, dists) [nq, k] numpy
        arrays, ranked by (distance, row); dists float64, NOT squared (the convention of `rerank`).  With more than n features asked
        for, the tail holds id -1 (None for non-numeric ids) and NaN.  This is what the ADC search approximates."""
        import torch
        if not (q.is_cuda and q.is_contiguous() and q.dim() == 2 and q.dtype in (torch.float32, torch.float64)
                and q.shape[1] == self.feats.shape[1]):
            raise ValueError("q must be a contiguous float32/float64 [nq, D] tensor on the GPU with the features' width")
        nq, k = int(q.shape[0]), int(k)
        rows = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=q.device)
        dists = torch.empty((nq, max(k, 0)), dtype=torch.float64, device=q.device)
        code = lambda t: _lib.CIS_F32 if t.dtype == torch.float32 else _lib.CIS_F64
        _lib.check(_lib.lib().cis_exact_knn_dev(self.feats.data_ptr(), code(self.feats), int(self.feats.shape[0]), int(self.feats.shape[1]),
                                                q.data_ptr(), code(q), nq, k, 0, 0, rows.data_ptr(), dists.data_ptr(),
                                                torch.cuda.current_stream(q.device).cuda_stream))
        rows, dists = rows.cpu().numpy(), dists.cpu().numpy()
        if self._ids is None:
            return rows, dists
        table = np.asarray(self._ids)
        if table.dtype.kind in "iu":
            ids = np.where(rows >= 0, table[np.maximum(rows, 0)], -1)
        else:
            ids = np.where(rows >= 0, table.astype(object)[np.maximum(rows, 0)], None)
        return ids, dists

    # -- the same on the device: id -> row map, look-up and the fused re-rank (csrc/lopq_rerank.hip) ---------------------------
    def device_map(self, dev_ids=None):
        """Builds the device id -> feature row map on the current stream and caches it; returns (keys, rows) int64 tensors, or
        None for the identity (no ids were given: id = row, no table is built).  Integer ids are their own device ids; with
        other ids pass dev_ids, one int64 per row (LOPQSearcherHIP.device_ids_of(ids)).  A repeated id maps to its last row, a
        negative one to nothing.  Later calls on other streams wait for the build."""
        import torch
        if dev_ids is None:
            if self._ids is None:
                return None
            if self._dmap is not None:
                return self._dmap[:2]
            table = np.asarray(self._ids)
            if table.dtype.kind not in "iu" or table.ndim != 1 or (table.dtype.kind == "u" and table.size and int(table.max()) >= 1 << 63):
                raise ValueError("the ids are not int64 integers: pass dev_ids, one int64 device id per feature row "
                                 "(LOPQSearcherHIP.device_ids_of)")
            dev_ids = torch.as_tensor(np.ascontiguousarray(table, dtype=np.int64))
        elif not torch.is_tensor(dev_ids):
            dev_ids = torch.as_tensor(np.ascontiguousarray(dev_ids, dtype=np.int64))
        dev = self.feats.device
        dev_ids = dev_ids.to(dev).contiguous()
        n = int(self.feats.shape[0])
        if dev_ids.dtype != torch.int64 or tuple(dev_ids.shape) != (n,):
            raise ValueError("dev_ids must be int64, one per feature row (%d)" % n)
        cap = 2
        while cap < 2 * n:
            cap *= 2
        keys = torch.empty(cap, dtype=torch.int64, device=dev)
        rows = torch.empty(cap, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().cis_idmap_build_dev(dev_ids.data_ptr(), n, keys.data_ptr(), rows.data_ptr(), cap,
                                                  torch.cuda.current_stream(dev).cuda_stream))
        built = torch.cuda.Event()
        built.record(torch.cuda.current_stream(dev))
        self._dmap = (keys, rows, built)
        return keys, rows

    def _map_args(self, stream):
        """(keys pointer, rows pointer, cap) of the cached map, built on first use; `stream` is made to wait for the build."""
        if self._ids is None and self._dmap is None:
            return None, None, 0
        if self._dmap is None:
            self.device_map()
        keys, rows, built = self._dmap
        stream.wait_event(built)
        return keys.data_ptr(), rows.data_ptr(), int(keys.shape[0])

    def rows_of_dev(self, ids):
        """rows_of on the device: int64 tensor of ids' shape, -1 where the (device) id is unknown or negative.  No synchronise."""
        import torch
        if not (torch.is_tensor(ids) and ids.is_cuda and ids.is_contiguous() and ids.dtype == torch.int64):
            raise ValueError("ids must be a contiguous int64 tensor on the GPU")
        st = torch.cuda.current_stream(ids.device)
        keys, rows, cap = self._map_args(st)
        out = torch.empty_like(ids)
        _lib.check(_lib.lib().cis_idmap_lookup_dev(keys, rows, cap, int(self.feats.shape[0]), ids.data_ptr(), ids.numel(),
                                                   out.data_ptr(), st.cuda_stream))
        return out

    def rerank_dev(self, q, ids, adc, rerank_nb=None, max_returned=None, near_dup_th=None, out=None):
        """`rerank` with everything on the device and one kernel: q [nq, D] of the features' dtype, ids int64 [nq, L] device ids
        (< 0: no result), adc float64 [nq, L].  Returns a dict of tensors [nq, nb], nb = min(rerank_nb, L): ``ids`` (-1 padded),
        ``dists`` float64 (NaN padded; bit for bit the distances of `rerank`), ``src`` int32 (the place of a result in `ids`
        before the re-order) and ``n_kept`` int32 [nq].  Runs on the current stream; no synchronise, no host copy.  `out`: such
        a dict to write into.  nb > 1024 is a ValueError: the host `rerank` serves those."""
        import torch
        if not (q.is_cuda and q.is_contiguous() and q.dim() == 2 and q.dtype == self.feats.dtype and q.shape[1] == self.feats.shape[1]):
            raise ValueError("q must be a contiguous [nq, D] tensor on the GPU with the features' dtype and width")
        nq = int(q.shape[0])
        for t, dt, what in ((ids, torch.int64, "ids"), (adc, torch.float64, "adc")):
            if not (torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.dtype == dt and t.shape[0] == nq):
                raise ValueError("%s must be a contiguous %s [nq, L] tensor on the GPU" % (what, str(dt).split(".")[-1]))
        if ids.shape != adc.shape:
            raise ValueError("ids and adc must have the same shape")
        L = int(ids.shape[1])
        nb = L if rerank_nb is None else min(int(rerank_nb), L)
        if nb < 0 or (max_returned or 0) < 0:
            raise ValueError("rerank_nb and max_returned must be >= 0")
        dev = q.device
        shapes = (("ids", torch.int64, (nq, nb)), ("dists", torch.float64, (nq, nb)), ("src", torch.int32, (nq, nb)),
                  ("n_kept", torch.int32, (nq,)))
        if out is None:
            out = {k: torch.empty(shp, dtype=dt, device=dev) for k, dt, shp in shapes}
        for k, dt, shp in shapes:
            t = out[k]
            if not (t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == shp):
                raise ValueError("out[%r] must be a contiguous %s tensor of shape %r on the GPU" % (k, str(dt).split(".")[-1], shp))
        st = torch.cuda.current_stream(dev)
        keys, rows, cap = self._map_args(st)
        code = _lib.CIS_F32 if q.dtype == torch.float32 else _lib.CIS_F64
        _lib.check(_lib.lib().cis_rerank_select_dev(
            self.feats.data_ptr(), code, int(self.feats.shape[0]), int(self.feats.shape[1]), keys, rows, cap, q.data_ptr(), nq,
            ids.data_ptr(), adc.data_ptr(), L, nb, int(max_returned or 0), 0 if near_dup_th is None else 1,
            0.0 if near_dup_th is None else float(near_dup_th), out["ids"].data_ptr(), out["dists"].data_ptr(),
            out["src"].data_ptr(), out["n_kept"].data_ptr(), st.cuda_stream))
        return out

    def rerank(self, q, ids, adc_dists, rerank_nb=None, max_returned=None, near_dup_th=None):
        """Re-rank the results of a batch: ids / adc_dists [nq, L] (ids < 0 or NaN distance = no result).
        Returns per query (ids, dists) lists in the reference's final order."""
        ids = np.asarray(ids)
        adc = np.asarray(adc_dists, dtype=np.float64)
        nq, L = ids.shape
        nb = L if rerank_nb is None else min(int(rerank_nb), L)
        valid = ~np.isnan(adc[:, :nb]) if ids.dtype.kind not in "iu" else (ids[:, :nb] >= 0)
        rows = self.rows_of(ids[:, :nb])
        rows[~valid] = -1
        true_d = self.distances_dev(q, rows).cpu().numpy()
        out = []
        for qi in range(nq):
            d = np.where(np.isnan(true_d[qi]), adc[qi, :nb], true_d[qi])
            keep = [i for i in range(nb) if valid[qi, i] and (near_dup_th is None or d[i] <= near_dup_th)
                    and (not max_returned or i < max_returned)]
            order = np.argsort(d[keep], axis=0, kind="stable") if keep else []
            out.append(([ids[qi, keep[j]] for j in order], [float(d[keep[j]]) for j in order]))
        return out


class FeatureStore(object):
    """Features that live in HBM and change by kernels (include/cis_hip.h:cis_featstore_*; csrc/feat_store.hip): the reference's
    HBase feature table (``put`` per item, hbase_indexer_minimal.py:779-831) for a live index.  `put_dev` stores or overwrites
    rows by id, `remove_dev` takes them out again, `get_dev` gathers them, and `rerank_dev` / `rows_of_dev` / `search_exact`
    have the signatures and the results of ResidentFeatures', so LOPQSearcherHIP.search_rerank_dev(q, store, ...) takes a store
    where it takes a ResidentFeatures.

    Ids are DEVICE ids, int64 >= 0: an integer id is its own device id; for other ids (the reference's sha1_bbox strings) the
    caller maps with LOPQSearcherHIP.device_ids_of, after the insert that created their slots.  The store keeps ONE row per id,
    the last one put.  (The index's dedup only skips an id already in the same cell: an id whose new code lands in another cell
    is stored a second time there, as in the reference; its feature is the last one either way.)

    Rows [0, len) are dense.  A removal fills the holes below the new length with the rows from the tail, so after a removal
    the row order is not the insertion order, and `search_exact` breaks exact distance ties by row.  One store per device;
    calls on a store must be ordered by the caller's streams.  Nothing is persisted."""

    def __init__(self, D, dtype, reserve=0, device=None):
        import torch
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be torch.float32 or torch.float64")
        self.D, self.dtype = int(D), dtype
        self._code = _lib.CIS_F32 if dtype == torch.float32 else _lib.CIS_F64
        self._fs = None
        h = _lib.ctypes.c_void_p()
        # (the library comes first: without a GPU this is its loud failure, not torch's)
        _lib.check(_lib.lib().cis_featstore_create(_lib.ctypes.byref(h), self.D, self._code, int(reserve)))
        self._fs = h
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    # -- life cycle --------------------------------------------------------------------------------------------------------------
    def close(self):
        if self._fs:
            _lib.lib().cis_featstore_destroy(self._fs)
            self._fs = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._fs:
            raise ValueError("this feature store is closed")
        return self._fs

    def __len__(self):
        return int(_lib.lib().cis_featstore_size(self._handle()))

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device)

    def reserve(self, rows):
        """Room for `rows` rows and their table entries, so that later puts up to that size allocate nothing."""
        _lib.check(_lib.lib().cis_featstore_reserve(self._handle(), int(rows), self._stream().cuda_stream))

    def _view(self):
        """(feats, row_ids, keys, rows pointers, cap, n): borrowed, valid until the next put or reserve -- fetched per call."""
        c = _lib.ctypes
        f, ri, k, r = c.c_void_p(), c.c_void_p(), c.c_void_p(), c.c_void_p()
        cap, n = c.c_int64(0), c.c_int64(0)
        _lib.check(_lib.lib().cis_featstore_view(self._handle(), c.byref(f), c.byref(ri), c.byref(k), c.byref(r), c.byref(cap), c.byref(n)))
        return f.value, ri.value, k.value, r.value, int(cap.value), int(n.value)

    def table_capacity(self):
        """Slots of the id -> row table (a power of two)."""
        return self._view()[4]

    def _check_ids(self, ids, what="ids"):
        import torch
        if not (torch.is_tensor(ids) and ids.is_cuda and ids.is_contiguous() and ids.dtype == torch.int64 and ids.dim() == 1):
            raise ValueError("%s must be a contiguous int64 [n] tensor on the GPU" % what)

    # -- put / remove / get ------------------------------------------------------------------------------------------------------
    def put_dev(self, ids, feats):
        """Store feats [n, D] under the device ids [n] (tensors in HBM), by kernels on the current stream: a stored id is
        overwritten, a repeated id keeps its last row, ids < 0 are skipped.  Returns (new, skipped)."""
        self._check_ids(ids)
        if not (feats.is_cuda and feats.is_contiguous() and feats.dim() == 2 and feats.dtype == self.dtype
                and tuple(feats.shape) == (int(ids.shape[0]), self.D)):
            raise ValueError("feats must be a contiguous %s [%d, %d] tensor on the GPU" % (str(self.dtype).split(".")[-1], int(ids.shape[0]), self.D))
        new, skipped = _lib.c_int64(0), _lib.c_int64(0)
        _lib.check(_lib.lib().cis_featstore_put_dev(self._handle(), ids.data_ptr(), feats.data_ptr(), int(ids.shape[0]),
                                                    _lib.ctypes.byref(new), _lib.ctypes.byref(skipped), self._stream().cuda_stream))
        return int(new.value), int(skipped.value)

    def remove_dev(self, ids):
        """Remove the stored ids of the list (unknown, negative and repeated ones are ignored).  Returns the number removed."""
        self._check_ids(ids)
        removed = _lib.c_int64(0)
        _lib.check(_lib.lib().cis_featstore_remove_dev(self._handle(), ids.data_ptr(), int(ids.shape[0]), _lib.ctypes.byref(removed),
                                                       self._stream().cuda_stream))
        return int(removed.value)

    def get_dev(self, ids):
        """(feats [m, D], rows int64 [m]) of the device ids [m]: an unknown or negative id gives row -1 and a row of zeros.
        No synchronise."""
        import torch
        self._check_ids(ids)
        m = int(ids.shape[0])
        feats = torch.empty((m, self.D), dtype=self.dtype, device=ids.device)
        rows = torch.empty(m, dtype=torch.int64, device=ids.device)
        _lib.check(_lib.lib().cis_featstore_get_dev(self._handle(), ids.data_ptr(), m, feats.data_ptr(), rows.data_ptr(),
                                                    self._stream().cuda_stream))
        return feats, rows

    def _upload_ids(self, ids):
        import torch
        return torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)).to(self.device)

    def put(self, ids, feats):
        """put_dev on host arrays (uploaded first)."""
        import torch
        a = np.ascontiguousarray(feats, dtype=np.float32 if self.dtype == torch.float32 else np.float64).reshape(-1, self.D)
        return self.put_dev(self._upload_ids(ids), torch.as_tensor(a).to(self.device))

    def remove(self, ids):
        """remove_dev on a host array of device ids."""
        return self.remove_dev(self._upload_ids(ids))

    def row_ids(self):
        """The device id of every row [0, len): an int64 tensor, copied from the store's column on the current stream (the
        column itself moves when the rows grow, so no tensor is left pointing into it)."""
        return self.rows_dev(feats=False)[1]

    def rows_dev(self, first=0, count=None, feats=True):
        """(feats [count, D] or None, ids int64 [count]) of the rows [first, first + count) as they lie in the store, copied on the
        current stream (count=None: up to the last row)."""
        import torch
        first = int(first)
        count = len(self) - first if count is None else int(count)
        if first < 0 or count < 0:
            raise ValueError("first and count must be >= 0")
        f = torch.empty((count, self.D), dtype=self.dtype, device=self.device) if feats else None
        ids = torch.empty(count, dtype=torch.int64, device=self.device)
        _lib.check(_lib.lib().cis_featstore_rows_dev(self._handle(), first, count, None if f is None else f.data_ptr(), ids.data_ptr(),
                                                     self._stream().cuda_stream))
        return f, ids

    # -- what ResidentFeatures offers, on the store's own arrays --------------------------------------------------------------------
    def rows_of_dev(self, ids):
        """ResidentFeatures.rows_of_dev: int64 tensor of ids' shape, -1 where the id is not stored.  No synchronise."""
        import torch
        if not (torch.is_tensor(ids) and ids.is_cuda and ids.is_contiguous() and ids.dtype == torch.int64):
            raise ValueError("ids must be a contiguous int64 tensor on the GPU")
        _, _, keys, rows, cap, n = self._view()
        out = torch.empty_like(ids)
        _lib.check(_lib.lib().cis_idmap_lookup_dev(keys, rows, cap, n, ids.data_ptr(), ids.numel(), out.data_ptr(),
                                                   torch.cuda.current_stream(ids.device).cuda_stream))
        return out

    def rerank_dev(self, q, ids, adc, rerank_nb=None, max_returned=None, near_dup_th=None, out=None):
        """ResidentFeatures.rerank_dev on the store's rows and table as they are now (cis_featstore_view, fetched anew on every
        call): the same kernel, the same results.  A result whose id is not stored keeps its ADC distance."""
        import torch
        if not (q.is_cuda and q.is_contiguous() and q.dim() == 2 and q.dtype == self.dtype and q.shape[1] == self.D):
            raise ValueError("q must be a contiguous [nq, D] tensor on the GPU with the features' dtype and width")
        nq = int(q.shape[0])
        for t, dt, what in ((ids, torch.int64, "ids"), (adc, torch.float64, "adc")):
            if not (torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.dtype == dt and t.shape[0] == nq):
                raise ValueError("%s must be a contiguous %s [nq, L] tensor on the GPU" % (what, str(dt).split(".")[-1]))
        if ids.shape != adc.shape:
            raise ValueError("ids and adc must have the same shape")
        L = int(ids.shape[1])
        nb = L if rerank_nb is None else min(int(rerank_nb), L)
        if nb < 0 or (max_returned or 0) < 0:
            raise ValueError("rerank_nb and max_returned must be >= 0")
        dev = q.device
        shapes = (("ids", torch.int64, (nq, nb)), ("dists", torch.float64, (nq, nb)), ("src", torch.int32, (nq, nb)),
                  ("n_kept", torch.int32, (nq,)))
        if out is None:
            out = {k: torch.empty(shp, dtype=dt, device=dev) for k, dt, shp in shapes}
        for k, dt, shp in shapes:
            t = out[k]
            if not (t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == shp):
                raise ValueError("out[%r] must be a contiguous %s tensor of shape %r on the GPU" % (k, str(dt).split(".")[-1], shp))
        feats, _, keys, rows, cap, n = self._view()
        _lib.check(_lib.lib().cis_rerank_select_dev(
            feats, self._code, n, self.D, keys, rows, cap, q.data_ptr(), nq, ids.data_ptr(), adc.data_ptr(), L, nb,
            int(max_returned or 0), 0 if near_dup_th is None else 1, 0.0 if near_dup_th is None else float(near_dup_th),
            out["ids"].data_ptr(), out["dists"].data_ptr(), out["src"].data_ptr(), out["n_kept"].data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream))
        return out

    def distances_packed_dev(self, q, recs, off, cnt, rerank_nb):
        """The sharded re-rank, on the rank that owns the hits (cis_rerank_packed_dev): recs int64 [n, 4] are cis_hit records, list
        i is recs[off[i] : off[i] + cnt[i]] and belongs to query row q[i] (the packed layout of search_partial_packed_dev, or a
        dense [rows, L] answer with off = row * L).  Returns float64 [n], parallel to recs: the distance of `rerank` for the first
        `rerank_nb` records of every list whose id is stored here, NaN for the others.  Entries outside every list are left as
        they were allocated.  No synchronise.  rerank_nb > 1024 is a ValueError."""
        import torch
        if not (q.is_cuda and q.is_contiguous() and q.dim() == 2 and q.dtype == self.dtype and q.shape[1] == self.D):
            raise ValueError("q must be a contiguous [nq, D] tensor on the GPU with the features' dtype and width")
        nq = int(q.shape[0])
        if not (torch.is_tensor(recs) and recs.is_cuda and recs.is_contiguous() and recs.dtype == torch.int64 and recs.dim() == 2
                and recs.shape[1] == 4):
            raise ValueError("recs must be a contiguous int64 [n, 4] tensor on the GPU")
        for t, dt, what in ((off, torch.int64, "off"), (cnt, torch.int32, "cnt")):
            if not (torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == (nq,)):
                raise ValueError("%s must be a contiguous %s [nq] tensor on the GPU" % (what, str(dt).split(".")[-1]))
        nb = int(rerank_nb)
        if nb < 0 or nb > 1024:
            raise ValueError("rerank_nb must be in [0, 1024] on the device (rerank_nb = %d)" % nb)
        n_rec = int(recs.shape[0])
        true_d = torch.empty(n_rec, dtype=torch.float64, device=q.device)
        feats, _, keys, rows, cap, n = self._view()
        _lib.check(_lib.lib().cis_rerank_packed_dev(feats, self._code, n, self.D, keys, rows, cap, q.data_ptr(), nq, recs.data_ptr(),
                                                    n_rec, off.data_ptr(), cnt.data_ptr(), nb, true_d.data_ptr(),
                                                    torch.cuda.current_stream(q.device).cuda_stream))
        return true_d

    def search_exact(self, q, k):
        """ResidentFeatures.search_exact over the rows [0, len): (ids, dists) [nq, k] numpy arrays ranked by (distance, row), ids
        mapped through the store's id column (-1 / NaN padded).  After a removal the rows are not in insertion order: that is
        the order exact distance ties are broken in."""
        import torch
        if not (q.is_cuda and q.is_contiguous() and q.dim() == 2 and q.dtype in (torch.float32, torch.float64) and q.shape[1] == self.D):
            raise ValueError("q must be a contiguous float32/float64 [nq, D] tensor on the GPU with the features' width")
        nq, k = int(q.shape[0]), int(k)
        rows = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=q.device)
        dists = torch.empty((nq, max(k, 0)), dtype=torch.float64, device=q.device)
        feats, _, _, _, _, n = self._view()
        _lib.check(_lib.lib().cis_exact_knn_dev(feats, self._code, n, self.D, q.data_ptr(),
                                                _lib.CIS_F32 if q.dtype == torch.float32 else _lib.CIS_F64, nq, k, 0, 0,
                                                rows.data_ptr(), dists.data_ptr(), torch.cuda.current_stream(q.device).cuda_stream))
        table = self.row_ids().cpu().numpy()
        rows, dists = rows.cpu().numpy(), dists.cpu().numpy()
        if table.shape[0] == 0:
            return np.full_like(rows, -1), dists
        return np.where(rows >= 0, table[np.maximum(rows, 0)], -1), dists


def rerank_select_merged_dev(ids, adc, src_rec, true_d, rerank_nb=None, max_returned=None, near_dup_th=None):
    """The sharded re-rank, on the home rank (cis_rerank_select_merged_dev): ids int64 / adc float64 / src_rec int64 [nq, L] from
    lopq.search.merge_packed_src_dev, true_d float64 [n] the gathered distances of distances_packed_dev in the layout of the merged
    records.  A result's distance is true_d[src_rec], or its ADC distance where that is NaN.  Returns rerank_dev's dict: ``ids``,
    ``dists``, ``src`` (the place in the merged ADC list) [nq, nb] and ``n_kept`` [nq], nb = min(rerank_nb, L).  No synchronise;
    nb > 1024 is a ValueError."""
    import torch
    if not (torch.is_tensor(ids) and ids.is_cuda and ids.is_contiguous() and ids.dim() == 2 and ids.dtype == torch.int64):
        raise ValueError("ids must be a contiguous int64 [nq, L] tensor on the GPU")
    nq, L = int(ids.shape[0]), int(ids.shape[1])
    for t, dt, what in ((adc, torch.float64, "adc"), (src_rec, torch.int64, "src_rec")):
        if not (torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == (nq, L)):
            raise ValueError("%s must be a contiguous %s [nq, L] tensor on the GPU" % (what, str(dt).split(".")[-1]))
    if not (torch.is_tensor(true_d) and true_d.is_cuda and true_d.is_contiguous() and true_d.dtype == torch.float64):
        raise ValueError("true_d must be a contiguous float64 tensor on the GPU")
    nb = L if rerank_nb is None else min(int(rerank_nb), L)
    if nb < 0 or (max_returned or 0) < 0:
        raise ValueError("rerank_nb and max_returned must be >= 0")
    if nb > 1024:
        raise ValueError("the device re-ranking holds at most 1024 results per query (nb = %d): use the host rerank" % nb)
    dev = ids.device
    out = {"ids": torch.empty((nq, nb), dtype=torch.int64, device=dev), "dists": torch.empty((nq, nb), dtype=torch.float64, device=dev),
           "src": torch.empty((nq, nb), dtype=torch.int32, device=dev), "n_kept": torch.empty(nq, dtype=torch.int32, device=dev)}
    _lib.check(_lib.lib().cis_rerank_select_merged_dev(
        ids.data_ptr(), adc.data_ptr(), src_rec.data_ptr(), nq, L, true_d.data_ptr(), true_d.numel(), nb, int(max_returned or 0),
        0 if near_dup_th is None else 1, 0.0 if near_dup_th is None else float(near_dup_th), out["ids"].data_ptr(),
        out["dists"].data_ptr(), out["src"].data_ptr(), out["n_kept"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out
