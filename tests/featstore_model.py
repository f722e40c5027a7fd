"""A pure-Python model of the feature store's semantics (include/cis_hip.h:cis_featstore_*), over numpy arrays: the `put` loop
and the hole-filling rule of `remove`, written the slow and obvious way.  tests/test_feature_store.py holds the device store
against it byte for byte; the model itself is checked against hand-written cases there."""
import numpy as np


class FeatStoreModel(object):
    def __init__(self, D, dtype):
        self.D, self.dtype = int(D), np.dtype(dtype)
        self.feats = np.zeros((0, self.D), dtype=self.dtype)
        self.row_ids = np.zeros(0, dtype=np.int64)
        self.row = {}

    def __len__(self):
        return len(self.row)

    def put(self, ids, batch):
        """-> (new, skipped)"""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        batch = np.asarray(batch, dtype=self.dtype).reshape(ids.shape[0], self.D)
        new = skipped = 0
        feats, row_ids = list(self.feats), list(self.row_ids)
        for i in range(ids.shape[0]):
            k = int(ids[i])
            if k < 0:
                skipped += 1
                continue
            if k not in self.row:
                self.row[k] = len(self.row)
                feats.append(None)
                row_ids.append(k)
                new += 1
            feats[self.row[k]] = batch[i].copy()
            row_ids[self.row[k]] = k
        self.feats = np.array(feats, dtype=self.dtype).reshape(len(feats), self.D)
        self.row_ids = np.array(row_ids, dtype=np.int64)
        return new, skipped

    def remove(self, ids):
        """-> removed.  With k removed and n' = n - k: the holes are the removed rows below n', ascending; the movers are the kept
        rows at or above n', ascending; mover j goes to hole j."""
        n = len(self.row)
        gone = sorted({self.row[int(k)] for k in np.asarray(ids, dtype=np.int64).reshape(-1) if int(k) >= 0 and int(k) in self.row})
        k = len(gone)
        n2 = n - k
        holes = [r for r in gone if r < n2]
        movers = [r for r in range(n2, n) if r not in set(gone)]
        assert len(holes) == len(movers)
        for r in gone:
            del self.row[int(self.row_ids[r])]
        for h, m in zip(holes, movers):
            self.feats[h] = self.feats[m]
            self.row_ids[h] = self.row_ids[m]
            self.row[int(self.row_ids[h])] = h
        self.feats = self.feats[:n2].copy()
        self.row_ids = self.row_ids[:n2].copy()
        return k

    def rows_of(self, ids):
        return np.array([self.row.get(int(k), -1) if int(k) >= 0 else -1 for k in np.asarray(ids).reshape(-1)], dtype=np.int64)

    def get(self, ids):
        """-> (feats [m, D] with zero rows for unknown ids, rows [m])"""
        rows = self.rows_of(ids)
        out = np.zeros((rows.shape[0], self.D), dtype=self.dtype)
        if len(self.row):
            out[rows >= 0] = self.feats[rows[rows >= 0]]
        return out, rows
