"""Device-resident object-feature store: batches name images, a kernel gathers their rows (csrc/dfol_store.hip).

`BatchGQABoxFeaturesCollator.collate_object_features` reads every image's features out of the chunk files, concatenates
`[features, W, H, x, y, w, h]` on the host and the batch ships that matrix to the GPU: 822 KB per question at 100 objects x 2048 features,
which binds a stream of unseen batches to PCIe.  The store holds the chunk files' `features`, `bboxes` and the per-image `(W, H)` on the
device instead - the whole GQA corpus is ~122 GB of fp32, one MI355X has 288 GB - and a batch carries only an `ObjectFeatureRef`: the store
slot and object count of each of its images.  `ProgramBatch.to_cuda` resolves the ref into the same `[O, F + 6]` matrix, bit for bit.

A store built with `direct=True` resolves a ref into a `StoreRows` instead: the row numbers of the batch in the store's own table and its
six box columns (28 bytes per object).  The featurizer's first product then reads the table through the row numbers
(csrc/dfol_dense_wide.hip, ROWS) and the `[O, F + 6]` matrix is never written; whoever needs the matrix calls `StoreRows.materialize()`.

A store built with `featurized=True` (which implies the index form) also keeps the OUTPUT of a frozen featurizer for every row of its table:
`featurize(net)` runs the network over the table once, `StoreRows.objects(cache)` gathers a batch's cached rows beside their box positions
(dfol_store_objects_f32) and no featurizer product runs per batch.  The cache is keyed by the network's weight versions; `release_raw()`
then frees the raw features (a quarter of the memory is left at 2048 -> 512).

A store built with `feature_dtype="bf16"` (which implies the index form too) holds its features as bfloat16, each rounded to nearest even by the
dense kernels' own rounding (dfol_store_round_bf16): half the memory.  In the bf16 arithmetic (`mlp_math: bf16`) the featurizer's first product
and its weight gradient round every feature that way before they multiply, so there they read the table in place (dfol_linear_act_rows_bf16t_f32,
dfol_linear_wgrad_bias_rows_bf16t) and no result bit changes; every other consumer gets the `[O, F + 6]` fp32 matrix of the ROUNDED features
(dfol_gather_object_rows_bf16_f32) - reduced precision outside the bf16 arithmetic, never a default.  With DFOL_STORE_BF16_DIRECT=1 (opt-in,
read when a forward starts) the default arithmetic's inference reads the table in place as well: the wide kernel widens each stored value
exactly and splits it into the two fp16 pieces the matrix route would have built (dfol_linear_wide_rows_bf16t_h2_f32), so the matrix is never
written and no result bit changes - still on the ROUNDED features; a store whose every value is an fp16 value (`f16_exact`, one pass over the
table on first use) gets the two-product form of that kernel, again with the same bits.  With DFOL_STORE_BF16_TRAIN=1 (opt-in, read the same way) a featurizer that
TRAINS in the default arithmetic without an active Dropout reads the table in place too: the same forward product, and a weight gradient whose
dY keeps its three bf16 pieces while a table value is its own one piece (dfol_linear_wgrad_bias_rows_bf16t_x3: three products, not six) - the
matrix route's bits, no `[O, F + 6]` matrix.  Every other arithmetic, an active Dropout and DFOL_WGRAD_MATH=f32 keep the matrix.

Three kinds of object, by who may hold them:
  DeviceFeatureStore   main process only: the device tensors, `gather`.  Registers itself by id in this process' table.
  FeatureStoreIndex    `store.index`: host-only and picklable, image id -> (slot or -1, object count).  This is what a collator - and so
                       every DataLoader worker - gets; no device tensor is reachable from it.
  ObjectFeatureRef     what a collator puts in a ProgramBatch's `_object_features` when every image of the batch is resident.
"""

import json
import os
import uuid
import weakref
import zipfile

import numpy as np
import torch

from . import _lib

_STORES = weakref.WeakValueDictionary()        # store id -> DeviceFeatureStore of THIS process


class ObjectFeatureRef(object):
    """The images of one batch as rows of a store: `slots` [I] int32 (any order, repeats allowed) and `counts` [I] int32 objects each."""

    __slots__ = ("store_id", "slots", "counts", "_pinned")

    def __init__(self, store_id, slots, counts):
        self.store_id = store_id
        self.slots = np.ascontiguousarray(slots, np.int32)
        self.counts = np.ascontiguousarray(counts, np.int32)
        self._pinned = None

    def index_array(self):
        """[slot (I) | first output row of every image (I + 1)] int32: what the kernel reads, one upload."""
        off = np.zeros(len(self.counts) + 1, np.int64)
        np.cumsum(self.counts, out=off[1:])
        if off[-1] >= 2 ** 31:
            raise _lib.DfolError("feature store: %d object rows in one batch" % off[-1])
        return np.concatenate([self.slots, off.astype(np.int32)])

    def source_rows(self, max_obj):
        """[O] int32: the store-table row (slot * max_obj + j) behind every object row of the batch, images in the ref's order - what
        dfol_store_rows_f32 writes on the device, restated on the host."""
        check_row_space(int(self.slots.max()) + 1 if len(self.slots) else 1, max_obj)
        counts = np.minimum(self.counts.astype(np.int64), int(max_obj))
        first = np.repeat(self.slots.astype(np.int64) * int(max_obj), counts)
        within = np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)
        return (first + within).astype(np.int32)

    def pin_memory(self):
        self._pinned = torch.from_numpy(self.index_array()).pin_memory()
        return self

    def __getstate__(self):                     # (the pinned copy stays in the process that made it)
        return (self.store_id, self.slots, self.counts)

    def __setstate__(self, state):
        self.store_id, self.slots, self.counts = state
        self._pinned = None


def check_row_space(S, max_obj):
    """The index form names a store row by ONE int32 (slot * max_obj + j): a store of 2^31 rows or more is refused, as the kernel's host does."""
    if int(S) * int(max_obj) >= 2 ** 31:
        raise _lib.DfolError("feature store: S * max_obj = %d x %d rows do not fit int32 row numbers (< 2^31); build the store without direct=True"
                             % (int(S), int(max_obj)))


def featurizer_key(net):
    """What a cache of `net`'s outputs depends on: every parameter's storage and version (an optimizer step, a load_state_dict or any other
    in-place update bumps the version) and the arithmetic of the dense products."""
    return (tuple((p.data_ptr(), p._version) for p in net.parameters()), _lib._dense_math())


class FeaturizedRows(object):
    """The host side of a featurized store's cache: the rows, the key they were computed under, and whether the raw features behind them are
    still there.  No device call: a DeviceFeatureStore owns one and asks it."""

    def __init__(self):
        self.rows, self.key, self.raw_released, self.builds = None, None, False, 0

    def valid_for(self, net):
        return self.rows is not None and self.key == featurizer_key(net)

    def set(self, net, rows):
        self.rows, self.key = rows, featurizer_key(net)
        self.builds += 1
        return rows

    def release_raw(self):
        if self.rows is None:
            raise _lib.DfolError("feature store: release_raw() before featurize(net): there is no cache to serve batches from")
        self.raw_released = True

    def need_raw(self, what):
        if self.raw_released:
            raise _lib.DfolError("feature store: %s needs the raw features, which release_raw() has freed; build the store again" % what)


FEATURIZE_BLOCK_ROWS = 32768                   # rows per product of featurize(): 256 of the wide kernel's 128-row blocks, a shape it takes by default


class FeatureStoreIndex(object):
    """Which images a store holds, and where: host-only, picklable, safe to hand to DataLoader workers."""

    def __init__(self, store_id, feature_dim, max_obj, table):
        self.store_id, self.F, self.max_obj = store_id, int(feature_dim), int(max_obj)
        self._table = table                     # image id -> (slot or -1, object count)

    def __len__(self):
        return len(self._table)

    def __contains__(self, image_id):
        return self._table.get(image_id, (-1, 0))[0] >= 0

    def get(self, image_id):
        return self._table.get(image_id, (-1, 0))

    def ref(self, image_ids):
        """ObjectFeatureRef of a batch's images, or None when one of them is not resident (the batch then takes the host route)."""
        entries = [self._table.get(im, (-1, 0)) for im in image_ids]
        if any(slot < 0 for slot, _ in entries):
            return None
        return ObjectFeatureRef(self.store_id, [slot for slot, _ in entries], [n for _, n in entries])


def _chunk_path(directory, prefix, i):
    base = os.path.join(directory, "%s_%d" % (prefix, i))
    for ext in (".npz", ".h5"):
        if os.path.exists(base + ext):
            return base + ext
    raise FileNotFoundError(base + ".npz|.h5")


def _array_shape(path, arrays, name):
    """Shape of one array of a container without reading it (an .npz member's header; an .h5 dataset knows its shape)."""
    if path.endswith(".npz"):
        with zipfile.ZipFile(path) as z, z.open(name + ".npy") as fh:
            version = np.lib.format.read_magic(fh)
            read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
            return tuple(read(fh)[0])
    return tuple(arrays[name].shape)


class StoreLayout(object):
    """The host half of building a store: the chunk files' shapes (read from their headers, no array is loaded) and the info JSON."""

    def __init__(self, object_h5_path, file_prefix, chunk_num, object_info_json_path, feature_itemsize=4):
        from .data import _open_arrays
        with open(object_info_json_path, "r") as f:
            self.info = json.load(f)
        self.paths = [_chunk_path(object_h5_path, file_prefix, i) for i in range(chunk_num)]
        self.shapes = []
        for p in self.paths:
            arrays = _open_arrays(p)
            self.shapes.append(tuple(int(d) for d in _array_shape(p, arrays, "features")))
            if hasattr(arrays, "close"):
                arrays.close()
        self.max_obj, self.F = self.shapes[0][1:]
        if any(s[1:] != (self.max_obj, self.F) for s in self.shapes):
            raise _lib.DfolError("feature store: chunk files of different [max_obj, F]: %s" % sorted(set(s[1:] for s in self.shapes)))
        self.feature_row_bytes = int(feature_itemsize) * self.max_obj * self.F         # (4: fp32 features; 2: a bf16 store's)
        self.row_bytes = self.feature_row_bytes + 4 * (self.max_obj * 4 + 2)           # features, boxes and (W, H) of one image
        self.chunk_bytes = [s[0] * self.row_bytes for s in self.shapes]

    def index(self, store_id, max_bytes=None):
        """-> (FeatureStoreIndex, sizes [S, 2] fp32, first slot of every resident chunk [resident + 1]).  max_bytes: whole chunks in file
        order for as long as they fit; None: every chunk."""
        resident, used = 0, 0
        while resident < len(self.paths) and (max_bytes is None or used + self.chunk_bytes[resident] <= max_bytes):
            used += self.chunk_bytes[resident]
            resident += 1
        base = np.concatenate([[0], np.cumsum([s[0] for s in self.shapes[:resident]])]).astype(np.int64)
        sizes = np.zeros((int(base[-1]), 2), np.float32)
        table = {}
        for image_id, inf in self.info.items():
            c, n = int(inf["file"]), int(inf["objectsNum"])
            if c < resident:
                if not (0 <= int(inf["idx"]) < self.shapes[c][0] and 0 <= n <= self.max_obj):
                    raise _lib.DfolError("feature store: image %s (idx %s, %d objects) does not fit chunk %d %s"
                                         % (image_id, inf["idx"], n, c, self.shapes[c]))
                slot = int(base[c]) + int(inf["idx"])
                sizes[slot] = (inf["width"], inf["height"])
                table[image_id] = (slot, n)
            else:
                table[image_id] = (-1, n)
        return FeatureStoreIndex(store_id, self.F, self.max_obj, table), sizes, base


class DeviceFeatureStore(object):
    """The chunk files of a BatchGQABoxFeaturesCollator (`<prefix>_<i>.npz|.h5`: `features [chunk, max_obj, F]`, `bboxes [chunk, max_obj, 4]`
    as x1, y1, x2, y2; the info JSON: image id -> {objectsNum, width, height, idx, file}) resident on `device` as three fp32 tensors:
    `features [S, max_obj, F]`, `boxes [S, max_obj, 4]` as stored, `sizes [S, 2]`; slot = rows of the chunks before the image's + `idx`.

    max_bytes=None: the whole corpus, which must fit in 80 % of the device memory that is free now - otherwise DfolError, nothing is
    allocated.  max_bytes=N: whole chunks in file order for as long as they fit in N bytes; batches that name an image of a later chunk
    take the host route (FeatureStoreIndex.ref -> None).

    direct=True (opt-in; recorded on the store only - index, refs and collators are the same): `resolve`, i.e. ProgramBatch.to_cuda, hands the
    batch on as a StoreRows (`rows`) and the featurizer reads the store's rows in place where its first product is one the wide kernel takes;
    every other consumer materialises the matrix as before.

    featurized=True (opt-in; implies direct=True): the store also caches a frozen featurizer's output for every row of its table - `featurize`,
    `cached_for` - and a batch whose featurizer does not train gets its object matrix from the cache (`StoreRows.objects`); `release_raw()` then
    frees the raw features.

    feature_dtype="bf16" (opt-in; implies direct=True; "f32" is the default): `features` is bfloat16 - every feature rounded to nearest even on
    the device, chunk by chunk (one fp32 chunk of extra memory while the store is built) - and `nbytes`, max_bytes and the free-memory check
    count the bytes actually held.  F must be a multiple of 4 (8-byte rows).  Under `mlp_math: bf16` the featurizer's first layer reads the
    table in place, forward and weight gradient, with the fp32 store's bits; every other arithmetic and consumer gets the gathered matrix of the
    rounded features.  Not with featurized=True: a cache over a bf16 table is not built."""

    def __init__(self, object_h5_path, file_prefix, chunk_num, object_info_json_path, device, max_bytes=None, direct=False, featurized=False,
                 feature_dtype="f32"):
        from .data import _open_arrays
        if feature_dtype not in ("f32", "bf16"):
            raise _lib.DfolError("feature store: feature_dtype must be 'f32' or 'bf16', got %r" % (feature_dtype,))
        bf16 = feature_dtype == "bf16"
        if bf16 and featurized:
            raise _lib.DfolError("feature store: feature_dtype='bf16' with featurized=True: a cache of featurizer rows over a bf16 table is not built")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DfolError("a feature store lives on a GPU (got device %s)" % (device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        lay = StoreLayout(object_h5_path, file_prefix, chunk_num, object_info_json_path, feature_itemsize=2 if bf16 else 4)
        if bf16 and lay.F % 4 != 0:
            raise _lib.DfolError("feature store: feature_dtype='bf16' needs F %% 4 == 0 (8-byte rows of bfloat16), the chunk files have F = %d" % lay.F)
        if max_bytes is None:
            need, free = sum(lay.chunk_bytes), int(torch.cuda.mem_get_info(self.device)[0])
            if need > 0.8 * free:
                raise _lib.DfolError("feature store: the corpus needs %d bytes, 80 %% of the free device memory is %d bytes (%d free); "
                                     "pass max_bytes= for a partial store" % (need, int(0.8 * free), free))
        self.id = uuid.uuid4().hex
        self.index, sizes, base = lay.index(self.id, max_bytes)
        S, max_obj, F = int(base[-1]), lay.max_obj, lay.F
        self.features = torch.empty((S, max_obj, F), dtype=torch.bfloat16 if bf16 else torch.float32, device=self.device)
        self.boxes = torch.empty((S, max_obj, 4), dtype=torch.float32, device=self.device)
        for c in range(len(base) - 1):             # one chunk on the host at a time
            arrays = _open_arrays(lay.paths[c])
            chunk = torch.from_numpy(np.ascontiguousarray(arrays["features"][...], np.float32))
            if bf16:                               # through one fp32 chunk on the device, rounded into the table's slice by the kernels' own rule
                with torch.cuda.device(self.device):
                    _lib.store_round_bf16(chunk.to(self.device), self.features[base[c]:base[c + 1]])
            else:
                self.features[base[c]:base[c + 1]].copy_(chunk)
            self.boxes[base[c]:base[c + 1]].copy_(torch.from_numpy(np.ascontiguousarray(arrays["bboxes"][...], np.float32)))
            if hasattr(arrays, "close"):
                arrays.close()
        self.sizes = torch.from_numpy(sizes).to(self.device)
        self.S, self.max_obj, self.F = S, max_obj, F
        self.featurized = bool(featurized)
        self.feature_dtype = feature_dtype
        self._f16_exact = None                             # (the certificate of a bf16 table, computed on first use: `f16_exact`)
        self.direct = bool(direct) or self.featurized or bf16
        self._featurized = FeaturizedRows()
        self.cache_nbytes = 0                              # (the cache of featurize(), beside `nbytes` of chunk data)
        if self.direct:
            check_row_space(S, max_obj)
        self.nbytes = S * lay.row_bytes
        self.resident_chunks = len(base) - 1
        _STORES[self.id] = self

    @property
    def f16_exact(self):
        """A bf16 store's certificate that every feature it holds is finite and an fp16 value (dfol_store_bf16_is_f16): the wide kernel's
        two-product form then gives the three-product bits.  Computed on first use - under DFOL_STORE_BF16_DIRECT=1 or DFOL_STORE_BF16_TRAIN=1 when the first batch's rows
        are resolved, never at construction - and cached: the table does not change after upload.  False for an fp32 store.  Not inside a
        stream capture (it waits for the device)."""
        if self._f16_exact is None:
            self._f16_exact = self.feature_dtype == "bf16" and self.features is not None and _lib.store_bf16_is_f16(self.features)
        return self._f16_exact

    def upload_index(self, ref):
        """The ref's index arrays on the device, checked against the store first (the kernel trusts them): -> int32 [slot (I) | obj_off (I + 1)].
        A few hundred bytes, from the ref's own pinned copy (ProgramBatch.pin_memory) or through the pinned staging ring.  Not inside a stream
        capture: a graph would bake in one batch's images - its owner gathers between replays."""
        if ref.store_id != self.id:
            raise _lib.DfolError("feature store %s asked for a ref of store %s" % (self.id, ref.store_id))
        slots, counts = ref.slots, ref.counts
        I = len(slots)
        if len(counts) != I or (I and (slots.min() < 0 or slots.max() >= self.S or counts.min() < 0 or counts.max() > self.max_obj)):
            raise _lib.DfolError("feature store: a ref outside the store (S = %d, max_obj = %d)" % (self.S, self.max_obj))
        if torch.cuda.is_current_stream_capturing():
            raise _lib.DfolError("feature store: gather uploads the batch's index arrays and cannot run inside a stream capture; "
                                 "call it between replays, with out= the captured batch's feature buffer")
        with torch.cuda.device(self.device):
            idx = torch.empty(2 * I + 1, dtype=torch.int32, device=self.device)
            if ref._pinned is not None:
                idx.copy_(ref._pinned, non_blocking=True)
            elif I:
                host = ref.index_array()
                if host.nbytes <= (1 << 20):
                    from . import host_util
                    host_util.ring_for(self.device).copy_to(idx.view(torch.uint8), host)
                else:
                    idx.copy_(torch.from_numpy(host))
            else:
                idx.zero_()
        return idx

    def gather(self, ref, out=None, index=None):
        """The batch's `[O, F + 6]` object matrix on the store's device, launched on the current stream.  out=: written into that buffer
        (rows of unit column stride, at least F + 6 columns, O rows) - how the owner of a GraphedForward / GraphedTrainStep serves new scenes
        into its captured batch, BETWEEN replays (see upload_index).  index=: the result of an earlier upload_index(ref)."""
        self._featurized.need_raw("gather")
        O = int(ref.counts.sum(dtype=np.int64))
        if out is None:
            out = torch.empty((O, self.F + 6), dtype=torch.float32, device=self.device)
        elif out.dim() != 2 or out.shape[0] != O or out.shape[1] < self.F + 6 or out.device != self.device:
            raise _lib.DfolError("feature store: out= must be [%d, >= %d] on %s, got %s on %s" % (O, self.F + 6, self.device, tuple(out.shape), out.device))
        idx = self.upload_index(ref) if index is None else index
        I = len(ref.slots)
        if idx.numel() != 2 * I + 1:
            raise _lib.DfolError("feature store: index= is not this ref's")
        if O == 0:
            return out
        with torch.cuda.device(self.device):
            _lib.gather_object_rows(self.features, self.boxes, self.sizes, idx[:I], idx[I:], out)
        return out


    # ---- the cache of a frozen featurizer's rows (featurized=True) -----------------------------------------------------------------------
    def featurize(self, net):
        """Run the featurizer network `net` (BatchGQABoxFeaturizer._featurizer_network) over every row of the store's table -> the cache
        [S * max_obj, W] fp32, kept under the key of net's weight versions.  Blocks of FEATURIZE_BLOCK_ROWS rows: the first layer by the direct
        route's own product (linear_wide_rows over the table, an identity row block), later layers by linear_act - a row's result does not depend
        on the rows beside it, so a batch's cached rows are the direct route's.  Refused (DfolError) where the direct route would step aside -
        no network, another first-layer width, another arithmetic - inside a stream capture, and after release_raw().  An fp16 range flag
        raises as it would from a forward."""
        from . import ops as L
        from .interpreter import store_layers_of
        if torch.cuda.is_current_stream_capturing():
            raise _lib.DfolError("feature store: featurize() builds the cache of featurizer rows and cannot run inside a stream capture; build it "
                                 "(or run one eager forward) before the capture")
        from .interpreter import active_dropout
        drop = active_dropout(net)
        if drop is not None:
            raise _lib.DfolError("feature store: featurize(): nn.%r of the featurizer network is in training mode: its rows differ from step to "
                                 "step and cannot be cached; put the featurizer in eval() (or use dropout: 0)" % (drop,))
        self._featurized.need_raw("featurize() for new featurizer weights")
        if self.features.dtype != torch.float32:
            raise _lib.DfolError("feature store: featurize(): a cache of featurizer rows over a bf16 table (feature_dtype='bf16') is not built")
        layers, why = store_layers_of(net, self.F, FEATURIZE_BLOCK_ROWS)
        if layers is None:
            raise _lib.DfolError("feature store: featurize(): %s" % why)
        rows, W = self.S * self.max_obj, int(layers[-1][0].weight.shape[0])
        table = self.features.view(rows, self.F)
        with torch.no_grad(), torch.cuda.device(self.device):
            cache = torch.empty((rows, W), dtype=torch.float32, device=self.device)
            ident = torch.arange(min(rows, FEATURIZE_BLOCK_ROWS), dtype=torch.int32, device=self.device)
            watch = _lib.RangeWatch(self.device)
            try:
                for r0 in range(0, rows, FEATURIZE_BLOCK_ROWS):
                    n = min(FEATURIZE_BLOCK_ROWS, rows - r0)
                    x = None
                    for k, (lin, act) in enumerate(layers):
                        out = cache[r0:r0 + n] if k == len(layers) - 1 else None
                        x = _lib.linear_wide_rows(table[r0:], ident[:n], lin.weight, lin.bias, act, out) if k == 0 else \
                            L.linear_act(x, lin.weight, lin.bias, act, out)
            finally:
                check = watch.finish()
            check()                                        # (waits for the products: the cache is whole, and in range, when this returns)
        _lib.note("feature_store_featurize")
        self.cache_nbytes = rows * W * 4
        return self._featurized.set(net, cache)

    def cached_for(self, net, build=False):
        """The cache if it was computed with net's current weights, else None.  build=True: a missing or stale cache is built first (once per
        weight version) - None then means that featurize() does not take this network; after release_raw() that, like a stale cache, raises."""
        if self._featurized.valid_for(net):
            return self._featurized.rows
        if not build:
            return None
        from .interpreter import store_layers_of
        if store_layers_of(net, self.F, FEATURIZE_BLOCK_ROWS)[0] is None and not self._featurized.raw_released:
            return None                                    # (the batch goes on as a direct store's)
        return self.featurize(net)                         # (raises inside a capture and after release_raw())

    def release_raw(self):
        """Free the raw features once a cache exists: the store then serves frozen-featurizer batches only, in a quarter of the memory at
        2048 -> 512.  Explicit and one-way: `gather`, `StoreRows.materialize`, a featurizer that trains and `featurize` for new weights raise a
        DfolError naming this call."""
        self._featurized.release_raw()
        if self.features is not None:
            self.nbytes -= self.features.numel() * self.features.element_size()
            self.features = None
        return self

    def rows(self, ref, out=None, index=None):
        """The batch in index form -> StoreRows (src_row [O] int32, box6 [O, 6], this store's table), one small launch on the current stream.
        out=: an existing StoreRows of this store with the same image and object counts, rewritten in place - how the owner of a captured forward
        serves a new scene BETWEEN replays: like upload_index, not inside a stream capture.  index=: an earlier upload_index(ref)."""
        check_row_space(self.S, self.max_obj)
        if self.feature_dtype == "bf16" and self._f16_exact is None and (_lib.store_bf16_direct() or _lib.store_bf16_train()):
            self.f16_exact                                 # (the certificate, here and not in a forward: a captured one cannot wait for the device)
        O, I = int(ref.counts.sum(dtype=np.int64)), len(ref.slots)
        idx = self.upload_index(ref) if index is None else index
        if idx.numel() != 2 * I + 1:
            raise _lib.DfolError("feature store: index= is not this ref's")
        if out is None:
            out = StoreRows(self, torch.empty(O, dtype=torch.int32, device=self.device), torch.empty((O, 6), dtype=torch.float32, device=self.device), idx)
        else:
            if not isinstance(out, StoreRows) or out.store is not self or out._index is None or out.O != O or out._index.numel() != 2 * I + 1:
                raise _lib.DfolError("feature store: out= must be a StoreRows of this store with %d images and %d objects" % (I, O))
            if torch.cuda.is_current_stream_capturing():
                raise _lib.DfolError("feature store: rows(out=) rewrites a captured batch's rows and cannot run inside a stream capture; "
                                     "call it between replays")
            out._index.copy_(idx)                      # (materialize() gathers through it)
        if O:
            with torch.cuda.device(self.device):
                _lib.store_rows(self.boxes, self.sizes, idx[:I], idx[I:], out.src_row, out.box6)
        return out


class StoreRows(object):
    """A batch's objects as rows of a `direct` store: `src_row` [O] int32 rows of `table` (the store's features viewed as [S * max_obj, F]) and
    `box6` [O, 6] = (W, H, x, y, w, h), the matrix's last six columns.  Stands where the `[O, F + 6]` matrix stood in a ProgramBatch: it has its
    shape, device and dtype for the size checks, and `materialize()` for every consumer that needs the tensor."""

    def __init__(self, store, src_row, box6, index, parent=None, picked=None):
        self.store, self.src_row, self.box6 = store, src_row, box6
        self.table = None if store.features is None else store.features.view(store.S * store.max_obj, store.F)      # (None: release_raw())
        self.bf16_ld = int(self.table.stride(0)) if self.table is not None and self.table.dtype == torch.bfloat16 else None     # a bf16 table's row stride
        self.O = int(src_row.numel())
        self._index = index                                # device [slot (I) | obj_off (I + 1)] of the ref, or None: a selection of `parent`'s rows
        self._parent, self._picked = parent, picked

    shape = property(lambda self: (self.O, self.store.F + 6))
    device = property(lambda self: self.store.device)
    dtype = torch.float32
    is_cuda = True

    def size(self, dim=None):
        return torch.Size(self.shape) if dim is None else self.shape[dim]

    def materialize(self, out=None):
        """The `[O, F + 6]` matrix, bit for bit `store.gather(ref)` (the same kernel through the same index arrays)."""
        st = self.store
        st._featurized.need_raw("StoreRows.materialize() (a featurizer that trains, a stale cache, or a consumer of the [O, F + 6] matrix)")
        if self._index is None:                            # selected rows: the parent's matrix, then the selection - what build_scene did before
            m = self._parent.materialize().index_select(0, self._picked)
            return m if out is None else out.copy_(m)
        if out is None:
            out = torch.empty((self.O, st.F + 6), dtype=torch.float32, device=st.device)
        elif out.dim() != 2 or out.shape[0] != self.O or out.shape[1] < st.F + 6 or out.device != st.device:
            raise _lib.DfolError("feature store: out= must be [%d, >= %d] on %s, got %s on %s" % (self.O, st.F + 6, st.device, tuple(out.shape), out.device))
        I = (self._index.numel() - 1) // 2
        if self.O:
            with torch.cuda.device(st.device):
                _lib.gather_object_rows(st.features, st.boxes, st.sizes, self._index[:I], self._index[I:], out)
        return out

    def objects(self, cache, out=None):
        """The object matrix `[O, W + 4]` of the batch from a featurized store's cache (`store.featurize(net)` / `cached_for(net)`): the cached
        rows of src_row beside the box positions of box6, one launch (dfol_store_objects_f32).  A selection of rows has it too."""
        st = self.store
        if cache.dim() != 2 or cache.shape[0] != st.S * st.max_obj or cache.device != st.device:
            raise _lib.DfolError("feature store: cache must be [%d, W] on %s, got %s on %s" % (st.S * st.max_obj, st.device, tuple(cache.shape), cache.device))
        with torch.cuda.device(st.device):
            return _lib.store_objects(cache, self.src_row, self.box6, out)

    def select_rows(self, rows):
        """The StoreRows of rows `rows` (int64 device tensor, repeats allowed) of this one: the two small arrays composed, no feature row moved."""
        return StoreRows(self.store, self.src_row.index_select(0, rows), self.box6.index_select(0, rows), None, parent=self, picked=rows)


def resolve(ref, device):
    """ProgramBatch.to_cuda's step: the ref's matrix - or, from a `direct` store, its StoreRows - from the store registered under its id in this
    process."""
    store = _STORES.get(ref.store_id)
    if store is None:
        raise _lib.DfolError("no feature store %s in this process (a store serves the process that built it)" % ref.store_id)
    dev = torch.device(device)
    if dev.type != "cuda" or (dev.index is not None and dev.index != store.device.index):
        raise _lib.DfolError("feature store %s lives on %s, the batch goes to %s" % (ref.store_id, store.device, device))
    return store.rows(ref) if store.direct else store.gather(ref)
