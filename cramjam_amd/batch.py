"""Batch extension: many independent chunks per call (what the GPU is for).  Host buffers in, host
buffers out; chunks shard round-robin over the given engines (one per GPU), no collective."""
from concurrent.futures import ThreadPoolExecutor

from . import _native as N

_engines = {}


def _engine(device):
    if device not in _engines:
        _engines[device] = N.Engine(device)
    return _engines[device]


def _shard(devices, n, work):
    """index i -> devices[i mod G], one thread per device.  work(device, idx) -> a tuple of lists with one entry per index of idx each;
    returns the same tuple of lists for all n indices, in the caller's order"""
    devices = list(devices) if devices is not None else [0]
    G = len(devices)
    if G == 1:
        return work(devices[0], range(n))
    shards = [range(g, n, G) for g in range(G)]
    with ThreadPoolExecutor(G) as ex:
        parts = list(ex.map(work, devices, shards))
    cols = tuple([None] * n for _ in parts[0])
    for idx, part in zip(shards, parts):
        for col, p in zip(cols, part):
            for k, i in enumerate(idx):
                col[i] = p[k]
    return cols


def _pick(seq, idx):
    return seq if len(idx) == len(seq) else [seq[i] for i in idx]


def _run(what, op, flags, inputs, out_caps, devices, out=None, kind=N.BLOCKS, params=None, extra=None):
    """kind: N.BLOCKS (what = a CODEC_*), N.FRAMES (a FORMAT_*), N.BLOSC (params: the bytes of a cj_blosc_params, b"" = decompress),
    N.DICT (what = CODEC_LZ4_BLOCK, params: the dictionary, any bytes-like, borrowed) or N.DEFLATE / N.DEFLATE_COMPRESS (what = a DEFLATE_*), N.ZSTD / N.ZSTD_COMPRESS (what = ZSTD_FRAMES), N.BGZF (what = 0), N.ORC (what = an ORC_*, extra: the block size) or N.PARQUET (what = a PARQUET_*).
    out: results + memoryviews into it (one writable buffer, chunk i behind chunk i - 1's capacity): no object per output"""
    n = len(inputs)
    tail = {"dictionary": params} if kind is N.DICT else {"extra": extra} if kind.extra else {"params": params}
    if out is None:
        return _shard(devices, n, lambda dev, idx: _engine(dev).batch_host(what, op, flags, _pick(inputs, idx), _pick(out_caps, idx), kind, **tail))
    offsets, run = [], 0
    for c in out_caps:
        offsets.append(run); run += int(c)
    mv = memoryview(out).cast("B")
    res, = _shard(devices, n, lambda dev, idx: (_engine(dev).batch_host_into(what, op, flags, _pick(inputs, idx), _pick(out_caps, idx), out,
                                                                             _pick(offsets, idx), kind, **tail),))
    return res, [mv[offsets[i]:offsets[i] + max(res[i], 0)] for i in range(n)]


def _sizes_first(sizes, run):
    """a decode without capacities: `sizes` are the size query's answers — a chunk it accepts gets exactly its size as capacity, a chunk it
    rejects the query's code as its result and an empty output"""
    res, outs = run([max(s, 0) for s in sizes])
    bad = [i for i, s in enumerate(sizes) if s < 0]
    if bad:
        res = list(res)
        outs = list(outs)
        for i in bad:
            res[i], outs[i] = sizes[i], outs[i][:0]
    return res, outs


def lz4_decompress_blocks(blocks, output_lens=None, store_size=False, devices=None, out=None, dictionary=None):
    """decode many LZ4 blocks; returns (results, outputs) with results[i] = length or a negative CJ_E_* code.
    output_lens=None: the sizes are asked for first (lz4_block_sizes: the prefix, or for raw blocks the walk of their token chains):
    a block the query accepts gets exactly its size as capacity, a block it rejects gets the query's code as its result and an empty
    output.  The input then crosses the link TWICE (once for the query, once for the decode): 16 384 x 64 KiB chunks decode at
    0.52 of the rate (75.7 ms against 39.7 ms) of a call that passes output_lens — pass the lengths where the container stores them.
    out: ONE writable buffer (bytearray, numpy array) of at least sum(output_lens) bytes — the outputs are then memoryviews into it
    (chunk i behind chunk i - 1's capacity) instead of new `bytes` objects: the C-ABI's host rate without an allocation per chunk.
    dictionary: bytes-like — the ONE dictionary every block of the call was written against (LZ4_loadDict + LZ4_compress_fast_continue;
    only its last 64 KiB count).  Such a batch always runs one wavefront per block.  None: no dictionary."""
    flags = N.FLAG_LZ4_SIZE_PREFIX if store_size else 0
    kind = N.BLOCKS if dictionary is None else N.DICT
    run = lambda caps: _run(N.CODEC_LZ4_BLOCK, N.OP_DECOMPRESS, flags, blocks, caps, devices, out, kind, dictionary)
    if output_lens is not None:
        return run(output_lens)
    return _sizes_first(lz4_block_sizes(blocks, store_size, devices, dictionary), run)


def lz4_compress_blocks(chunks, store_size=True, devices=None, out=None, dictionary=None):
    """out: as in lz4_decompress_blocks; it has to hold sum(compress_block_bound(len(chunk))) bytes.
    dictionary: bytes-like — every chunk may refer to its last 64 KiB (what LZ4_decompress_safe_usingDict reads, and
    lz4_decompress_blocks(..., dictionary=...)); chunks of at most 65 536 bytes, a longer one gets -1 as its result."""
    L = N.lib()
    caps = [L.cj_lz4_block_compress_bound(len(c), 1 if store_size else 0) for c in chunks]
    return _run(N.CODEC_LZ4_BLOCK, N.OP_COMPRESS, N.FLAG_LZ4_SIZE_PREFIX if store_size else 0, chunks, caps, devices, out,
                N.BLOCKS if dictionary is None else N.DICT, dictionary)


def snappy_decompress_raw_many(blocks, devices=None, out=None):
    L = N.lib()
    import ctypes as C
    caps = []
    for b in blocks:
        b = bytes(b)
        caps.append(max(L.cj_snappy_raw_decompress_len(C.cast(C.c_char_p(b), C.c_void_p), len(b)), 0))
    return _run(N.CODEC_SNAPPY_RAW, N.OP_DECOMPRESS, 0, blocks, caps, devices, out)


def snappy_compress_raw_many(chunks, devices=None, out=None):
    L = N.lib()
    caps = [L.cj_snappy_raw_max_compress_len(len(c)) for c in chunks]
    return _run(N.CODEC_SNAPPY_RAW, N.OP_COMPRESS, 0, chunks, caps, devices, out)


# ---- batches of framed streams: one LZ4 frame / Snappy framed stream per entry (cj_frame_batch_host) ----------------------------
# result[i] and the bytes are what cramjam_amd.lz4.decompress / .compress and cramjam_amd.snappy.decompress / .compress give for that
# stream alone (the C exports' error codes instead of exceptions); output_lens: per-stream capacities (default: the bound of each stream).
def _addr_len(b):
    import numpy as np
    a = np.frombuffer(b, dtype=np.uint8)
    return _C.c_void_p(a.ctypes.data if a.size else None), a.size


def lz4_decompress_frames(frames, output_lens=None, devices=None, out=None):
    """decode many LZ4 frames; returns (results, outputs) as lz4_decompress_blocks"""
    if output_lens is None:
        L = N.lib()
        output_lens = [max(L.cj_lz4_frame_decompress_bound(*_addr_len(f)), 0) for f in frames]
    return _run(N.FORMAT_LZ4_FRAME, N.OP_DECOMPRESS, 0, frames, output_lens, devices, out, N.FRAMES)


def lz4_compress_frames(buffers, devices=None, out=None):
    """one LZ4 frame per buffer (64 KiB independent blocks, content checksum); out: as in lz4_decompress_blocks, it has to hold
    sum(cj_lz4_frame_compress_bound(len(buffer))) bytes"""
    L = N.lib()
    return _run(N.FORMAT_LZ4_FRAME, N.OP_COMPRESS, 0, buffers, [L.cj_lz4_frame_compress_bound(len(memoryview(b).cast("B"))) for b in buffers],
                devices, out, N.FRAMES)


def snappy_decompress_framed_many(streams, output_lens=None, devices=None, out=None):
    """decode many Snappy framed streams"""
    if output_lens is None:
        L = N.lib()
        output_lens = [max(L.cj_snappy_frame_decompress_len(*_addr_len(f)), 0) for f in streams]
    return _run(N.FORMAT_SNAPPY_FRAMED, N.OP_DECOMPRESS, 0, streams, output_lens, devices, out, N.FRAMES)


def snappy_compress_framed_many(buffers, devices=None, out=None):
    """one Snappy framed stream per buffer"""
    L = N.lib()
    return _run(N.FORMAT_SNAPPY_FRAMED, N.OP_COMPRESS, 0, buffers, [L.cj_snappy_frame_max_compress_len(len(memoryview(b).cast("B"))) for b in buffers],
                devices, out, N.FRAMES)


# ---- device-resident batches: no host copy, no ctypes at the call site ---------------------------------------------------------
# Every buffer argument is any object that exposes `__cuda_array_interface__` (torch tensors on ROCm, cupy arrays, numba device
# arrays) or `__dlpack__` (anything else that lives in HBM); torch is never imported here.  The reference's API is one Python call
# per buffer (/root/reference/src/lz4.rs:78-131, src/snappy.rs:52-78); this is the same call for a batch that already sits in
# HBM: chunk i is inp[in_off[i] : in_off[i] + in_len[i]] and decodes / encodes into out[out_off[i] : out_off[i] + out_cap[i]].
import ctypes as _C


class _DLDevice(_C.Structure):
    _fields_ = [("device_type", _C.c_int32), ("device_id", _C.c_int32)]


class _DLDataType(_C.Structure):
    _fields_ = [("code", _C.c_uint8), ("bits", _C.c_uint8), ("lanes", _C.c_uint16)]


class _DLTensor(_C.Structure):
    _fields_ = [("data", _C.c_void_p), ("device", _DLDevice), ("ndim", _C.c_int32), ("dtype", _DLDataType),
                ("shape", _C.POINTER(_C.c_int64)), ("strides", _C.POINTER(_C.c_int64)), ("byte_offset", _C.c_uint64)]


class _DLManagedTensor(_C.Structure):
    pass


_DLManagedTensor._fields_ = [("dl_tensor", _DLTensor), ("manager_ctx", _C.c_void_p),
                             ("deleter", _C.CFUNCTYPE(None, _C.POINTER(_DLManagedTensor)))]
_kDLCPU, _kDLCUDA, _kDLCUDAHost, _kDLROCM, _kDLROCMHost, _kDLCUDAManaged = 1, 2, 3, 10, 11, 13


class _DevView:
    """pointer + byte size of a contiguous device buffer, keeping its owner alive"""
    __slots__ = ("ptr", "nbytes", "itemsize", "count", "device", "_owner", "_capsule")

    def __init__(self, obj):
        self._owner, self._capsule, self.device = obj, None, None
        cai = getattr(obj, "__cuda_array_interface__", None)
        if cai is not None:
            shape, strides, typestr = tuple(cai["shape"]), cai.get("strides"), cai["typestr"]
            self.itemsize = int(typestr[2:])
            self.count = 1
            for s in shape:
                self.count *= int(s)
            if strides is not None and self.count:
                want, run = [], self.itemsize
                for s in reversed(shape):
                    want.append(run); run *= int(s)
                if tuple(strides) != tuple(reversed(want)):
                    raise ValueError("cramjam_amd.batch: device buffers must be contiguous")
            self.ptr = int(cai["data"][0]) if self.count else 0
            dev = getattr(obj, "device", None)
            # torch: .device.index; cupy: .device.id (round-5 advisor: a cupy buffer on GPU N fell back to engine 0)
            self.device = (getattr(dev, "index", None) if getattr(dev, "index", None) is not None else getattr(dev, "id", None)) if dev is not None else None
        elif hasattr(obj, "__dlpack__"):
            cap = obj.__dlpack__()
            api = _C.pythonapi
            api.PyCapsule_GetPointer.restype, api.PyCapsule_GetPointer.argtypes = _C.c_void_p, [_C.py_object, _C.c_char_p]
            p = api.PyCapsule_GetPointer(cap, b"dltensor")
            mt = _C.cast(p, _C.POINTER(_DLManagedTensor)).contents
            t = mt.dl_tensor
            if t.device.device_type not in (_kDLCUDA, _kDLROCM, _kDLCUDAManaged):
                raise ValueError("cramjam_amd.batch: the buffer is not in device memory (DLPack device type %d)" % t.device.device_type)
            if t.dtype.lanes != 1:
                raise ValueError("cramjam_amd.batch: vector dtypes are not supported")
            self.itemsize = t.dtype.bits // 8
            self.count = 1
            for k in range(t.ndim):
                self.count *= int(t.shape[k])
            if t.strides and self.count:
                run = 1
                for k in reversed(range(t.ndim)):
                    if int(t.shape[k]) != 1 and int(t.strides[k]) != run:
                        raise ValueError("cramjam_amd.batch: device buffers must be contiguous")
                    run *= int(t.shape[k])
            self.ptr = (int(t.data or 0) + int(t.byte_offset)) if self.count else 0
            self.device = int(t.device.device_id)
            self._capsule = (cap, mt)          # consumed when this view is released
        else:
            raise TypeError("cramjam_amd.batch: expected a device buffer (an object with __cuda_array_interface__ or __dlpack__), got %s"
                            % type(obj).__name__)
        self.nbytes = self.count * self.itemsize

    def release(self):
        if self._capsule is not None:
            cap, mt = self._capsule
            self._capsule = None
            if mt.deleter:
                mt.deleter(_C.pointer(mt))      # we are the consumer of the capsule: its deleter is ours to call, once
            _C.pythonapi.PyCapsule_SetName.argtypes = [_C.py_object, _C.c_char_p]
            _C.pythonapi.PyCapsule_SetName(cap, b"used_dltensor")


def _is_device_obj(x):
    return hasattr(x, "__cuda_array_interface__") or (hasattr(x, "__dlpack__") and not hasattr(x, "__array_interface__") and not isinstance(x, (list, tuple)))


class _DeviceCall:
    """What the device-resident calls share: the NULL-stream refusal, the views of the caller's buffers, the engine of their device,
    64-bit metadata (device arrays in place, host sequences uploaded for this call), the result array, the wait and the clean-up."""

    def __init__(self, stream, sync):
        if stream is not None and int(stream) == 0:
            raise ValueError("cramjam_amd.batch: the NULL stream (torch's default stream has handle 0) cannot be named through the C-ABI, where NULL means "
                             "the engine's own stream — run the producer on a torch.cuda.Stream() and pass its .cuda_stream, or leave stream=None and synchronize")
        self.stream, self.sync, self.views, self.temps, self.n, self.eng, self.own_result = stream, sync, [], [], None, None, False

    def buffer(self, obj):
        v = _DevView(obj)
        self.views.append(v)
        return v

    def engine(self, device, *views):
        if device is None:
            device = next((v.device for v in views if v.device is not None), 0)
        self.eng = _engine(device)
        return self.eng

    def meta(self, x, name):
        import numpy as np
        if _is_device_obj(x):
            v = self.buffer(x)
            if v.itemsize != 8:
                raise TypeError("cramjam_amd.batch: %s must hold 64-bit integers" % name)
            cnt, ptr = v.count, v.ptr
        else:                                   # a host sequence: uploaded for this call
            a = np.ascontiguousarray(np.asarray(x, dtype=np.uint64))
            cnt = a.size
            ptr = self.eng.alloc(max(a.nbytes, 8))
            self.temps.append(ptr)
            self.eng.h2d(ptr, a)
            self.sync = True
        if self.n is None:
            self.n = cnt
        elif cnt != self.n:
            raise ValueError("cramjam_amd.batch: %s has %d entries, expected %d" % (name, cnt, self.n))
        return ptr

    def result(self, result):
        self.own_result = result is None
        if self.own_result:
            ptr = self.eng.alloc(max(8 * self.n, 8))
            self.temps.append(ptr)
            self.sync = True
            return ptr
        vr = self.buffer(result)
        if vr.itemsize != 8 or vr.count != self.n:
            raise ValueError("cramjam_amd.batch: result must hold %d 64-bit integers" % self.n)
        return vr.ptr

    def finish(self, p_res, result):
        if self.sync:
            if self.stream is not None:
                N.check(N.lib().cj_stream_sync(self.eng.h, self.stream))
            else:
                self.eng.sync()
        if self.own_result:
            return self.eng.d2h(p_res, 8 * self.n, "int64")
        return result

    def close(self):
        for p in self.temps:
            self.eng.free(p)
        for v in self.views:
            v.release()


def _device_batch(kind, what, op, flags, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync, params=None, dictionary=None, extra=None):
    """dictionary (LZ4 blocks only): a device buffer — the batch goes through N.DICT with (its address, its length) behind result"""
    call = _DeviceCall(stream, sync)
    try:
        vin, vout = call.buffer(inp), call.buffer(out)
        eng = call.engine(device, vin, vout)
        if dictionary is not None:
            vd = call.buffer(dictionary)
            kind, params = N.DICT, (vd.ptr or None, vd.nbytes)
        i = (vin.ptr, call.meta(in_off, "in_off"), call.meta(in_len, "in_len"))
        o = (vout.ptr, call.meta(out_off, "out_off"), call.meta(out_cap, "out_cap"))
        p_res = call.result(result)
        N.check(getattr(N.lib(), kind.device)(*kind.device_args(eng.h, what, op, flags, call.n, i, o, p_res, params, stream, extra)))
        return call.finish(p_res, result)
    finally:
        call.close()


def _device_sizes(kind, what, flags, inp, in_off, in_len, result, device, stream, sync, dictionary=None, extra=None):
    call = _DeviceCall(stream, sync)
    try:
        vin = call.buffer(inp)
        eng = call.engine(device, vin)
        dict_len = 0
        if dictionary is not None:                  # (only its length enters the walk)
            kind, dict_len = N.DICT, call.buffer(dictionary).nbytes
        p_in_off, p_in_len = call.meta(in_off, "in_off"), call.meta(in_len, "in_len")
        p_res = call.result(result)
        N.check(getattr(N.lib(), kind.sizes_device)(*kind.sizes_args(eng.h, what, flags, call.n, (vin.ptr, p_in_off, p_in_len, p_res), (stream,), dict_len, extra)))
        return call.finish(p_res, result)
    finally:
        call.close()


def lz4_decompress_blocks_device(inp, in_off, in_len, out, out_off, out_cap, store_size=False, result=None, device=None, stream=None, sync=True,
                                 dictionary=None):
    """Decode a batch of LZ4 blocks that already sits in HBM (reference call per buffer: src/lz4.rs:78-95).

    inp / out: device byte buffers (torch tensor, cupy array, anything with __cuda_array_interface__ or __dlpack__);
    in_off, in_len, out_off, out_cap: 64-bit integer arrays of one entry per chunk — device arrays are used in place, host
    sequences / numpy arrays are uploaded; result: optional device int64 array that receives the decoded length of every chunk
    (or a negative CJ_E_* code).  Returns `result`, or — when it was None — a numpy int64 array with the same content.
    stream: a hipStream_t handle as an int (a torch.cuda.Stream().cuda_stream; not the default stream, whose handle 0 means "the engine's own" here) to order the
    batch behind the producer of the buffers; without it the batch runs on the engine's own stream and the caller makes sure the
    buffers are ready (torch.cuda.synchronize()).  sync=False returns right after submission (device-resident metadata and result
    only).  In a process that also uses torch, import torch FIRST: both link libamdhip64.so.7, torch loads its own copy by path, and
    two HIP runtimes in one process do not share a device.
    dictionary: a device byte buffer — the one dictionary of the batch, as in lz4_decompress_blocks."""
    return _device_batch(N.BLOCKS, N.CODEC_LZ4_BLOCK, N.OP_DECOMPRESS, N.FLAG_LZ4_SIZE_PREFIX if store_size else 0,
                         inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync, dictionary=dictionary)


def lz4_compress_blocks_device(inp, in_off, in_len, out, out_off, out_cap, store_size=True, result=None, device=None, stream=None, sync=True,
                               dictionary=None):
    """Compress a device-resident batch into LZ4 blocks (src/lz4.rs:113-131); out_cap[i] >= cramjam.lz4.compress_block_bound(in_len[i]).
    dictionary: a device byte buffer, as in lz4_compress_blocks (chunks of at most 65 536 bytes)."""
    return _device_batch(N.BLOCKS, N.CODEC_LZ4_BLOCK, N.OP_COMPRESS, N.FLAG_LZ4_SIZE_PREFIX if store_size else 0,
                         inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync, dictionary=dictionary)


def snappy_decompress_raw_many_device(inp, in_off, in_len, out, out_off, out_cap, result=None, device=None, stream=None, sync=True):
    """Decode a device-resident batch of Snappy raw blocks (src/snappy.rs:52-59)."""
    return _device_batch(N.BLOCKS, N.CODEC_SNAPPY_RAW, N.OP_DECOMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


def snappy_compress_raw_many_device(inp, in_off, in_len, out, out_off, out_cap, result=None, device=None, stream=None, sync=True):
    """Compress a device-resident batch into Snappy raw blocks (src/snappy.rs:70-78); out_cap[i] >= cramjam.snappy.compress_raw_max_len(in_len[i])."""
    return _device_batch(N.BLOCKS, N.CODEC_SNAPPY_RAW, N.OP_COMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


# ---- device-resident batches of framed streams (cj_frame_batch_device): the same arguments; stream i is inp[in_off[i] : + in_len[i]] and
# its output goes to out[out_off[i] : + out_cap[i]].  The call waits for the stream once (it reads back the block counts / in_len).
def lz4_decompress_frames_device(inp, in_off, in_len, out, out_off, out_cap, result=None, device=None, stream=None, sync=True):
    """Decode a device-resident batch of LZ4 frames (result[i] as cramjam_amd.lz4.decompress of frame i with that capacity)."""
    return _device_batch(N.FRAMES, N.FORMAT_LZ4_FRAME, N.OP_DECOMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


def lz4_compress_frames_device(inp, in_off, in_len, out, out_off, out_cap, result=None, device=None, stream=None, sync=True):
    """One LZ4 frame per device-resident buffer; out_cap[i] >= cj_lz4_frame_compress_bound(in_len[i])."""
    return _device_batch(N.FRAMES, N.FORMAT_LZ4_FRAME, N.OP_COMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


def snappy_decompress_framed_many_device(inp, in_off, in_len, out, out_off, out_cap, result=None, device=None, stream=None, sync=True):
    """Decode a device-resident batch of Snappy framed streams."""
    return _device_batch(N.FRAMES, N.FORMAT_SNAPPY_FRAMED, N.OP_DECOMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


def snappy_compress_framed_many_device(inp, in_off, in_len, out, out_off, out_cap, result=None, device=None, stream=None, sync=True):
    """One Snappy framed stream per device-resident buffer; out_cap[i] >= cj_snappy_frame_max_compress_len(in_len[i])."""
    return _device_batch(N.FRAMES, N.FORMAT_SNAPPY_FRAMED, N.OP_COMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


# ---- decoded sizes (cj_batch_sizes_* / cj_frame_batch_sizes_*): what out_off / out_cap of the calls above are computed from -----------
# result[i] = the decoded size of chunk i, or a negative CJ_E_* code.  Same buffer / metadata / stream / result conventions as the
# device-resident calls above — but these only ENQUEUE: with device-resident metadata, a result tensor and sync=False nothing waits,
# and the query may sit in front of the decode on the same stream.  The two-call pattern on torch tensors:
#
#     side = torch.cuda.Stream()
#     with torch.cuda.stream(side):
#         res = torch.empty(n, dtype=torch.int64, device="cuda")
#         batch.lz4_block_sizes_device(comp, in_off, in_len, result=res, stream=side.cuda_stream, sync=False)
#         cap = res.clamp(min=0); off = cap.cumsum(0) - cap            # rejected chunks: capacity 0
#         out = torch.empty(int(cap.sum()), dtype=torch.uint8, device="cuda")      # (the one read-back: the allocation needs a number)
#         batch.lz4_decompress_blocks_device(comp, in_off, in_len, out, off, cap, result=res2, stream=side.cuda_stream)
#
# (cap = S is enough for blocks that came from an encoder; cap = S + 12, CJ_LZ4_SIZE_SLACK, for any block the query accepted.)
LZ4_SIZE_SLACK = 12


def lz4_block_sizes_device(inp, in_off, in_len, store_size=False, result=None, device=None, stream=None, sync=True, dictionary=None):
    """Decoded sizes of a device-resident batch of LZ4 blocks.  store_size=True: the u32 prefix of each block (header only).
    store_size=False (raw blocks: Parquet LZ4_RAW, ORC, Arrow IPC): the token chain of every block is walked to its end — the exact
    size the decoder produces, CJ_E_CORRUPT (-7) for a block it would reject with any capacity.
    dictionary: the device buffer of the batch's dictionary (only its length enters: matches may reach that far behind a block's start)."""
    return _device_sizes(N.BLOCKS, N.CODEC_LZ4_BLOCK, N.FLAG_LZ4_SIZE_PREFIX if store_size else 0, inp, in_off, in_len, result, device, stream, sync, dictionary)


def snappy_raw_sizes_device(inp, in_off, in_len, result=None, device=None, stream=None, sync=True):
    """Announced lengths of a device-resident batch of Snappy raw blocks (cramjam.snappy.decompress_raw_len of each; header only)."""
    return _device_sizes(N.BLOCKS, N.CODEC_SNAPPY_RAW, 0, inp, in_off, in_len, result, device, stream, sync)


def lz4_frame_bounds_device(inp, in_off, in_len, result=None, device=None, stream=None, sync=True):
    """cj_lz4_frame_decompress_bound of every frame of a device-resident batch: an upper bound of its decoded size (the content size
    where the frame stores one), 0 for a skippable frame, or its header error."""
    return _device_sizes(N.FRAMES, N.FORMAT_LZ4_FRAME, 0, inp, in_off, in_len, result, device, stream, sync)


def snappy_framed_sizes_device(inp, in_off, in_len, result=None, device=None, stream=None, sync=True):
    """cj_snappy_frame_decompress_len of every stream of a device-resident batch: its decoded length, or its first header-level error."""
    return _device_sizes(N.FRAMES, N.FORMAT_SNAPPY_FRAMED, 0, inp, in_off, in_len, result, device, stream, sync)


def _host_sizes(kind, what, flags, buffers, devices, dict_len=0, extra=None):
    """sharded like _run: buffer i -> engine i mod G"""
    import numpy as np

    def work(dev, idx):
        arrs = [np.frombuffer(buffers[i], dtype=np.uint8) for i in idx]          # borrowed, not copied
        k = len(arrs)
        ptrs = (_C.c_void_p * max(k, 1))(*[a.ctypes.data if a.size else None for a in arrs])
        lens = (_C.c_size_t * max(k, 1))(*[a.size for a in arrs])
        res = np.empty(k, np.int64)
        N.check(getattr(N.lib(), kind.sizes_host)(*kind.sizes_args(_engine(dev).h, what, flags, k, (ptrs, lens, res.ctypes.data), (), dict_len, extra)))
        return ([int(x) for x in res],)
    return _shard(devices, len(buffers), work)[0]


def lz4_block_sizes(blocks, store_size=False, devices=None, dictionary=None):
    """decoded sizes of many LZ4 blocks held on the host (list of ints; negative = CJ_E_* code), as lz4_block_sizes_device"""
    flags = N.FLAG_LZ4_SIZE_PREFIX if store_size else 0
    if dictionary is not None:
        return _host_sizes(N.DICT, N.CODEC_LZ4_BLOCK, flags, blocks, devices, memoryview(dictionary).nbytes)
    return _host_sizes(N.BLOCKS, N.CODEC_LZ4_BLOCK, flags, blocks, devices)


def snappy_raw_sizes(blocks, devices=None):
    return _host_sizes(N.BLOCKS, N.CODEC_SNAPPY_RAW, 0, blocks, devices)


def lz4_frame_bounds(frames, devices=None):
    return _host_sizes(N.FRAMES, N.FORMAT_LZ4_FRAME, 0, frames, devices)


def snappy_framed_sizes(streams, devices=None):
    return _host_sizes(N.FRAMES, N.FORMAT_SNAPPY_FRAMED, 0, streams, devices)


# ---- Blosc chunks (cj_blosc_batch_* / cj_blosc_chunk_sizes_*): LZ4 streams behind shuffle / bitshuffle -----------------------------
# One Blosc1-format chunk per entry (what Zarr / numcodecs, PyTables and bcolz store; cramjam_amd.blosc2 is the single-chunk case).
# result[i] = nbytes (decompress) / the chunk's size (compress) or a negative CJ_E_* code: -30 a malformed chunk, -31 one this
# library does not read (another compressor format, C-Blosc2's extended header), -7 a bad LZ4 stream, -6 / -2 a capacity too small.
# blosclz=True (reading calls; off by default): chunks whose streams are BloscLZ, c-blosc's default compressor, are read too
# (CJ_BLOSC_FLAG_READ_BLOSCLZ); zlib=True / zstd=True: so are chunks whose streams are zlib streams / Zstandard frames (c-blosc's cname
# "zlib" / "zstd"; CJ_BLOSC_FLAG_READ_ZLIB / _ZSTD).  One batch may mix all of them with LZ4 chunks.
def _blosc_params(typesize, filter, clevel, codec, blocksize):
    from . import blosc2
    return bytes(blosc2._params(typesize, clevel, filter, codec, blocksize))


def _chunk_nbytes(c, blosclz=False, zlib=False, zstd=False):
    """nbytes of a chunk on the host from its header alone, 0 for one that will be refused"""
    from . import blosc2
    rc, nbytes = blosc2._info_nbytes(*_addr_len(c), blosclz, zlib, zstd)
    return nbytes if rc == 0 else 0


def blosc_decompress_chunks(chunks, devices=None, out=None, blosclz=False, zlib=False, zstd=False):
    """decode many Blosc chunks; returns (results, outputs) as lz4_decompress_blocks.  The capacities are the chunks' own nbytes
    (read on the host from their headers); out: ONE writable buffer of at least their sum, the outputs are then views into it.
    blosclz=True / zlib=True / zstd=True: chunks whose streams are BloscLZ / zlib streams / Zstandard frames are decoded too (the
    default refuses them with -31)."""
    return _run(0, N.OP_DECOMPRESS, N.BLOSC.read_flags(blosclz, zlib, zstd), chunks, [_chunk_nbytes(c, blosclz, zlib, zstd) for c in chunks], devices, out,
                N.BLOSC, b"")


def blosc_compress_chunks(buffers, typesize, filter=1, clevel=5, codec=1, blocksize=0, devices=None, out=None):
    """one Blosc chunk per buffer: LZ4 streams behind `filter` (0 none, 1 shuffle, 2 bitshuffle; cramjam_amd.blosc2.Filter) over
    elements of `typesize` bytes.  out has to hold sum(len(buffer) + 32) bytes."""
    caps = [memoryview(b).nbytes + 32 for b in buffers]
    return _run(0, N.OP_COMPRESS, 0, buffers, caps, devices, out, N.BLOSC, _blosc_params(typesize, filter, clevel, codec, blocksize))


def blosc_chunk_sizes(chunks, devices=None, blosclz=False, zlib=False, zstd=False):
    """nbytes of many Blosc chunks held on the host (list of ints; negative = the header's CJ_E_* code); blosclz, zlib, zstd: as in
    blosc_decompress_chunks"""
    return _host_sizes(N.BLOSC, 0, N.BLOSC.read_flags(blosclz, zlib, zstd), chunks, devices)


def blosc_decompress_chunks_device(inp, in_off, in_len, out, out_off, out_cap, result=None, device=None, stream=None, sync=True, blosclz=False,
                                   zlib=False, zstd=False):
    """Decode a device-resident batch of Blosc chunks (arguments as lz4_decompress_frames_device; the call waits for the stream once).
    blosclz, zlib, zstd: as in blosc_decompress_chunks."""
    return _device_batch(N.BLOSC, 0, N.OP_DECOMPRESS, N.BLOSC.read_flags(blosclz, zlib, zstd), inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


def blosc_compress_chunks_device(inp, in_off, in_len, out, out_off, out_cap, typesize, filter=1, clevel=5, codec=1, blocksize=0,
                                 result=None, device=None, stream=None, sync=True):
    """One Blosc chunk per device-resident buffer; out_cap[i] >= in_len[i] + 32 always suffices."""
    from . import blosc2
    return _device_batch(N.BLOSC, 0, N.OP_COMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync,
                         blosc2._params(typesize, clevel, filter, codec, blocksize))


def blosc_chunk_sizes_device(inp, in_off, in_len, result=None, device=None, stream=None, sync=True, blosclz=False, zlib=False, zstd=False):
    """nbytes of every chunk of a device-resident batch after the header checks, or their error; enqueue-only like lz4_block_sizes_device.
    blosclz, zlib, zstd: as in blosc_decompress_chunks."""
    return _device_sizes(N.BLOSC, 0, N.BLOSC.read_flags(blosclz, zlib, zstd), inp, in_off, in_len, result, device, stream, sync)


# ---- DEFLATE streams (cj_deflate_batch_* / cj_deflate_batch_sizes_*): raw DEFLATE, zlib streams, gzip members; decode only -----------
# One stream per entry (ORC's zlib codec writes raw DEFLATE, Parquet GZIP pages are gzip members, numcodecs Zlib / GZip chunks are zlib
# / gzip streams).  result[i] = the decoded length or a negative CJ_E_* code: -40 invalid DEFLATE data, -41 a zlib / gzip header zlib
# refuses, -42 Adler-32 / CRC-32 / ISIZE mismatch, -43 the input ends inside the stream, -44 bytes behind the stream (a second gzip
# member included), -6 a capacity too small.  The size query does not verify checksums.
_DEFLATE_WRAP = {"raw": N.DEFLATE_RAW, "zlib": N.DEFLATE_ZLIB, "gzip": N.DEFLATE_GZIP}


def _deflate_wrap(wrapper):
    try:
        return _DEFLATE_WRAP[wrapper]
    except (KeyError, TypeError):
        raise ValueError("wrapper must be 'raw', 'zlib' or 'gzip', not %r" % (wrapper,)) from None


def deflate_sizes(streams, wrapper="raw", devices=None):
    """decoded sizes of many DEFLATE streams held on the host (list of ints; negative = CJ_E_* code): the decoder's walk without its
    stores — exact for a stream that is valid to its end; checksums are NOT verified here, gzip's ISIZE is not read"""
    return _host_sizes(N.DEFLATE, _deflate_wrap(wrapper), 0, streams, devices)


def deflate_decompress_many(streams, output_lens=None, wrapper="raw", devices=None, out=None):
    """decode many DEFLATE streams; returns (results, outputs) as lz4_decompress_blocks.  wrapper: "raw" (RFC 1951), "zlib" (RFC 1950) or
    "gzip" (RFC 1952, one member per stream).  output_lens=None: the sizes are asked for first (deflate_sizes; the input then crosses
    the link twice): a stream the query rejects gets the query's code as its result and an empty output."""
    wrap = _deflate_wrap(wrapper)
    run = lambda caps: _run(wrap, N.OP_DECOMPRESS, 0, streams, caps, devices, out, N.DEFLATE)
    if output_lens is not None:
        return run(output_lens)
    return _sizes_first(deflate_sizes(streams, wrapper, devices), run)


def deflate_decompress_many_device(inp, in_off, in_len, out, out_off, out_cap, wrapper="raw", result=None, device=None, stream=None, sync=True):
    """Decode a device-resident batch of DEFLATE streams (arguments as lz4_decompress_blocks_device); enqueue-only with device-resident
    metadata, a result tensor and sync=False."""
    return _device_batch(N.DEFLATE, _deflate_wrap(wrapper), N.OP_DECOMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


def deflate_sizes_device(inp, in_off, in_len, wrapper="raw", result=None, device=None, stream=None, sync=True):
    """Decoded sizes of a device-resident batch of DEFLATE streams, as deflate_sizes; enqueue-only like lz4_block_sizes_device."""
    return _device_sizes(N.DEFLATE, _deflate_wrap(wrapper), 0, inp, in_off, in_len, result, device, stream, sync)


# ---- Zstandard frames (cj_zstd_batch_* / cj_zstd_batch_sizes_*): decode --------------------------------------------------
# One entry is what one ZSTD_decompress call reads: one or more frames, skippable frames skipped, b"" decoding to b"".  result[i] = the
# decoded length or a negative CJ_E_* code: -50 a bad frame header (legacy frames included), -51 corrupt data, -52 content checksum,
# -53 truncated input or bytes behind the last frame, -54 the frame names a dictionary, -6 a capacity too small.
def zstd_sizes(frames, devices=None):
    """decoded sizes of many Zstandard chunks held on the host (list of ints; negative = CJ_E_* code): Frame_Content_Size where a frame
    carries it, else the walk of its blocks without its literals — exact for a chunk that is valid; the content checksum and what
    only a full decode finds are NOT verified here (include/cramjam_hip.h lists them)"""
    return _host_sizes(N.ZSTD, N.ZSTD_FRAMES, 0, frames, devices)


def zstd_decompress_many(frames, devices=None, out=None):
    """decode many Zstandard chunks; returns (results, outputs) as lz4_decompress_blocks.  The sizes are asked for first (zstd_sizes;
    the input then crosses the link twice): a chunk the query rejects gets the query's code as its result and an empty output."""
    run = lambda caps: _run(N.ZSTD_FRAMES, N.OP_DECOMPRESS, 0, frames, caps, devices, out, N.ZSTD)
    return _sizes_first(zstd_sizes(frames, devices), run)


def zstd_decompress_many_device(inp, in_off, in_len, out, out_off, out_cap, result=None, device=None, stream=None, sync=True):
    """Decode a device-resident batch of Zstandard chunks (arguments as lz4_decompress_blocks_device); enqueue-only with device-resident
    metadata, a result tensor and sync=False (a call that has to grow the engine's literal slots waits for their previous user)."""
    return _device_batch(N.ZSTD, N.ZSTD_FRAMES, N.OP_DECOMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


def zstd_sizes_device(inp, in_off, in_len, result=None, device=None, stream=None, sync=True):
    """Decoded sizes of a device-resident batch of Zstandard chunks, as zstd_sizes; enqueue-only like lz4_block_sizes_device."""
    return _device_sizes(N.ZSTD, N.ZSTD_FRAMES, 0, inp, in_off, in_len, result, device, stream, sync)


# ---- ... and into them (cj_deflate_compress_batch_* / cj_deflate_compress_bound) --------------------------------------
# One stream per buffer: independent pieces of at most 64 KiB, each one stored, fixed or dynamic block.  result[i] = the stream's length
# or a negative CJ_E_* code (-6: the capacity is too small; -1: a buffer above 0x7E000000 bytes).
def deflate_compress_bound(n, wrapper="raw"):
    """the capacity that always suffices for a buffer of n bytes (exact worst case of the layout; 0 above 0x7E000000).  No device."""
    return N.lib().cj_deflate_compress_bound(n, _deflate_wrap(wrapper))


def deflate_compress_many(buffers, wrapper="raw", devices=None, out=None):
    """one DEFLATE stream per buffer; returns (results, outputs) as lz4_compress_blocks.  wrapper: "raw", "zlib" or "gzip" — what
    deflate_decompress_many, zlib.decompress and gzip.decompress read.  out: as in lz4_decompress_blocks; it has to hold
    sum(deflate_compress_bound(len(buffer), wrapper)) bytes."""
    wrap, L = _deflate_wrap(wrapper), N.lib()
    caps = [L.cj_deflate_compress_bound(memoryview(b).nbytes, wrap) for b in buffers]
    return _run(wrap, N.OP_COMPRESS, 0, buffers, caps, devices, out, N.DEFLATE_COMPRESS)


def deflate_compress_many_device(inp, in_off, in_len, out, out_off, out_cap, wrapper="raw", result=None, device=None, stream=None, sync=True):
    """Compress a device-resident batch into DEFLATE streams (arguments as lz4_compress_blocks_device); out_cap[i] >=
    deflate_compress_bound(in_len[i], wrapper) always suffices.  Enqueue-only with device-resident metadata, a result tensor and
    sync=False (a call that has to grow the engine's record slots waits for their previous user)."""
    return _device_batch(N.DEFLATE_COMPRESS, _deflate_wrap(wrapper), N.OP_COMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


# ---- BGZF streams (cj_bgzf_batch_* / cj_bgzf_sizes_* / cj_bgzf_compress_bound): blocked gzip, both directions ----------
# One entry is a whole stream of any size — a BAM, BCF or `bgzip` file: gzip members of at most 64 KiB that state their own length, so
# every member of every stream is decoded (encoded) on its own.  result[i] = the decoded (the stream's) length or a negative CJ_E_*
# code: -43 / -41 from the walk over the members' heads (truncated; not BGZF — bytes behind the last member, zero padding too), then
# -6 when the members' ISIZE sum exceeds the capacity, then the first bad member's code in stream order (-40, -42, ...).
def bgzf_sizes(streams, devices=None):
    """decoded sizes of many BGZF streams held on the host (list of ints; negative = CJ_E_* code): the sum of the members' ISIZE fields
    from the walk alone — claims read from the trailers, verified only by the decode"""
    return _host_sizes(N.BGZF, 0, 0, streams, devices)


def bgzf_decompress_many(streams, output_lens=None, devices=None, out=None):
    """decode many BGZF streams, member-parallel; returns (results, outputs) as lz4_decompress_blocks.  output_lens=None: the sizes are
    asked for first (bgzf_sizes; the input then crosses the link twice): a stream the walk rejects gets the walk's code as its result
    and an empty output."""
    run = lambda caps: _run(0, N.OP_DECOMPRESS, 0, streams, caps, devices, out, N.BGZF)
    if output_lens is not None:
        return run(output_lens)
    return _sizes_first(bgzf_sizes(streams, devices), run)


def bgzf_decompress_many_device(inp, in_off, in_len, out, out_off, out_cap, result=None, device=None, stream=None, sync=True):
    """Decode a device-resident batch of BGZF streams (arguments as lz4_decompress_frames_device; the call waits for the stream once, for
    the streams' member counts)."""
    return _device_batch(N.BGZF, 0, N.OP_DECOMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


def bgzf_sizes_device(inp, in_off, in_len, result=None, device=None, stream=None, sync=True):
    """Decoded sizes of a device-resident batch of BGZF streams, as bgzf_sizes; enqueue-only like lz4_block_sizes_device."""
    return _device_sizes(N.BGZF, 0, 0, inp, in_off, in_len, result, device, stream, sync)


def bgzf_compress_bound(n):
    """the capacity that always suffices for a buffer of n bytes (the members' worst cases and the end-of-file marker; 0 above
    0x7E000000).  No device."""
    return N.lib().cj_bgzf_compress_bound(n)


def bgzf_compress_many(buffers, devices=None, out=None):
    """one BGZF stream per buffer — members of 65 280 input bytes, then the end-of-file marker: what bgzf_decompress_many, htslib and
    gzip.decompress read; returns (results, outputs) as lz4_compress_blocks.  out: as in lz4_decompress_blocks; it has to hold
    sum(bgzf_compress_bound(len(buffer))) bytes."""
    L = N.lib()
    caps = [L.cj_bgzf_compress_bound(memoryview(b).nbytes) for b in buffers]
    return _run(0, N.OP_COMPRESS, 0, buffers, caps, devices, out, N.BGZF)


def bgzf_compress_many_device(inp, in_off, in_len, out, out_off, out_cap, result=None, device=None, stream=None, sync=True):
    """Compress a device-resident batch into BGZF streams (arguments as lz4_compress_frames_device; the call waits for the stream once,
    for the buffers' lengths); out_cap[i] >= bgzf_compress_bound(in_len[i]) always suffices."""
    return _device_batch(N.BGZF, 0, N.OP_COMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


# ---- ... and into Zstandard frames (cj_zstd_compress_batch_* / cj_zstd_compress_bound) --------------------------------
# One frame per buffer: independent pieces of at most 64 KiB, each one RLE, Compressed or Raw block.  result[i] = the frame's length
# or a negative CJ_E_* code (-6: the capacity is too small; -1: a buffer above 0x7E000000 bytes).
def _zstd_flags(checksum):
    return N.ZSTD_FLAG_CHECKSUM if checksum else 0


def zstd_compress_bound(n, checksum=False):
    """the capacity that always suffices for a buffer of n bytes (exact worst case of the layout: every piece a Raw block; 0 above
    0x7E000000).  No device."""
    return N.lib().cj_zstd_compress_bound(n, _zstd_flags(checksum))


def zstd_compress_many(buffers, checksum=False, devices=None, out=None):
    """one Zstandard frame per buffer; returns (results, outputs) as lz4_compress_blocks.  checksum: a Content_Checksum (XXH64's low 32
    bits) behind the last block — what zstd_decompress_many and libzstd's ZSTD_decompress read and verify.  out: as in
    lz4_decompress_blocks; it has to hold sum(zstd_compress_bound(len(buffer), checksum)) bytes."""
    flags, L = _zstd_flags(checksum), N.lib()
    caps = [L.cj_zstd_compress_bound(memoryview(b).nbytes, flags) for b in buffers]
    return _run(N.ZSTD_FRAMES, N.OP_COMPRESS, flags, buffers, caps, devices, out, N.ZSTD_COMPRESS)


def zstd_compress_many_device(inp, in_off, in_len, out, out_off, out_cap, checksum=False, result=None, device=None, stream=None, sync=True):
    """Compress a device-resident batch into Zstandard frames (arguments as lz4_compress_blocks_device); out_cap[i] >=
    zstd_compress_bound(in_len[i], checksum) always suffices.  Enqueue-only with device-resident metadata, a result tensor and
    sync=False (a call that has to grow the engine's record and literal slots waits for their previous user)."""
    return _device_batch(N.ZSTD_COMPRESS, N.ZSTD_FRAMES, N.OP_COMPRESS, _zstd_flags(checksum), inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


# ---- ORC compression streams (cj_orc_batch_* / cj_orc_sizes_* / cj_orc_compress_bound): both directions -----------------
# One entry is a whole stream of an ORC file as it lies there (a data stream, an index stream, a stripe footer, the file footer):
# chunks behind 3-byte headers, each the codec's output for at most block_size raw bytes or those bytes as they are.  result[i] = the
# decoded (the stream's) length or a negative CJ_E_* code: -60 from the walk over the headers (truncated), then the first chunk's in
# stream order whose size query fails (the codec's code) or that holds more than block_size bytes (-61), then -6 when the sizes' sum
# exceeds the capacity, then the first bad chunk's code in stream order.  No call here is enqueue-only: each waits for the stream once.
_ORC_KIND = {"zlib": N.ORC_ZLIB, "snappy": N.ORC_SNAPPY, "lz4": N.ORC_LZ4, "zstd": N.ORC_ZSTD}


def _orc_kind(codec):
    try:
        return _ORC_KIND[codec]
    except (KeyError, TypeError):
        raise ValueError("codec must be 'zlib', 'snappy', 'lz4' or 'zstd', not %r" % (codec,)) from None


def orc_stream_sizes(streams, codec, block_size=262144, devices=None):
    """decoded sizes of many ORC compression streams held on the host (list of ints; negative = CJ_E_* code): the walk over the chunk
    headers and the codec's size query over every compressed chunk — ORC states no decoded length.  For "snappy" the chunks' sizes are
    their headers' claims, verified only by the decode."""
    return _host_sizes(N.ORC, _orc_kind(codec), 0, streams, devices, extra=block_size)


def orc_decompress_streams(streams, codec, block_size=262144, output_lens=None, devices=None, out=None):
    """decode many ORC compression streams, chunk-parallel; returns (results, outputs) as lz4_decompress_blocks.  codec: "zlib", "snappy",
    "lz4" or "zstd" (the file's PostScript.compression); block_size: its compressionBlockSize — no chunk may hold more.
    output_lens=None: the sizes are asked for first (orc_stream_sizes; the input then crosses the link twice): a stream the query
    rejects gets the query's code as its result and an empty output."""
    kind = _orc_kind(codec)
    run = lambda caps: _run(kind, N.OP_DECOMPRESS, 0, streams, caps, devices, out, N.ORC, extra=block_size)
    if output_lens is not None:
        return run(output_lens)
    return _sizes_first(orc_stream_sizes(streams, codec, block_size, devices), run)


def orc_compress_bound(n, block_size=262144):
    """the capacity a buffer of n bytes needs: n + 3 * ceil(n / block_size), every piece an original chunk — exact for incompressible
    input, 0 for an empty buffer (an empty stream); also 0 above 0x7E000000 or for a block_size outside 1 .. 262 144.  No device."""
    return N.lib().cj_orc_compress_bound(n, block_size)


def orc_compress_streams(buffers, codec, block_size=262144, devices=None, out=None):
    """one ORC compression stream per buffer — pieces of block_size bytes, each the codec's output or, where that is not shorter, the
    original bytes: what orc_decompress_streams and every ORC reader read; returns (results, outputs) as lz4_compress_blocks.  out: as
    in lz4_decompress_blocks; it has to hold sum(orc_compress_bound(len(buffer), block_size)) bytes."""
    kind, L = _orc_kind(codec), N.lib()
    caps = [L.cj_orc_compress_bound(memoryview(b).nbytes, block_size) for b in buffers]
    return _run(kind, N.OP_COMPRESS, 0, buffers, caps, devices, out, N.ORC, extra=block_size)


def orc_decompress_streams_device(inp, in_off, in_len, out, out_off, out_cap, codec, block_size=262144, result=None, device=None, stream=None, sync=True):
    """Decode a device-resident batch of ORC compression streams (arguments as lz4_decompress_frames_device; the call waits for the
    stream once, for the streams' chunk counts)."""
    return _device_batch(N.ORC, _orc_kind(codec), N.OP_DECOMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync, extra=block_size)


def orc_stream_sizes_device(inp, in_off, in_len, codec, block_size=262144, result=None, device=None, stream=None, sync=True):
    """Decoded sizes of a device-resident batch of ORC compression streams, as orc_stream_sizes.  NOT enqueue-only: the call waits for
    the stream once, for the streams' chunk counts."""
    return _device_sizes(N.ORC, _orc_kind(codec), 0, inp, in_off, in_len, result, device, stream, sync, extra=block_size)


def orc_compress_streams_device(inp, in_off, in_len, out, out_off, out_cap, codec, block_size=262144, result=None, device=None, stream=None, sync=True):
    """Compress a device-resident batch into ORC compression streams (arguments as lz4_compress_frames_device; the call waits for the
    stream once, for the buffers' lengths and capacities); out_cap[i] must be at least orc_compress_bound(in_len[i], block_size)."""
    return _device_batch(N.ORC, _orc_kind(codec), N.OP_COMPRESS, 0, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync, extra=block_size)


# ---- Parquet column chunks (cj_parquet_batch_* / cj_parquet_sizes_* / cj_parquet_pages_*): decode only ------------------
# One entry is a column chunk as it lies in the file: total_compressed_size bytes from dictionary_page_offset (data_page_offset where
# there is no dictionary page) — pages behind Thrift compact headers, each the codec's output or, for a V2 page, its levels and the
# codec's output for the values.  result[i] = the decoded length or a negative CJ_E_* code: -70 from the walk over the headers, then -6
# when the pages' stated sizes' sum exceeds the capacity, then the first page's code in page order (-72 a CRC mismatch, the decoder's
# code, -71 a page that decodes to less than it states).  The footer's total_uncompressed_size counts the header bytes too: it is an
# upper bound on the decoded length and always suffices as a capacity.
_PARQUET_CODEC = {"uncompressed": N.PARQUET_UNCOMPRESSED, "snappy": N.PARQUET_SNAPPY, "gzip": N.PARQUET_GZIP, "zstd": N.PARQUET_ZSTD, "lz4_raw": N.PARQUET_LZ4_RAW}


def _parquet_codec(codec):
    try:
        return _PARQUET_CODEC[codec]
    except (KeyError, TypeError):
        raise ValueError("codec must be 'uncompressed', 'snappy', 'gzip', 'zstd' or 'lz4_raw', not %r" % (codec,)) from None


def parquet_chunk_sizes(chunks, codec, devices=None):
    """decoded sizes of many Parquet column chunks held on the host (list of ints; negative = CJ_E_* code): the sum of the pages'
    uncompressed_page_size from the walk over the headers alone — claims, verified only by the decode.  The footer's
    total_uncompressed_size is this sum plus the header bytes, so it always suffices as a capacity."""
    return _host_sizes(N.PARQUET, _parquet_codec(codec), 0, chunks, devices)


def parquet_decompress_chunks(chunks, codec, output_lens=None, verify_crc=False, devices=None, out=None):
    """decode many Parquet column chunks, page-parallel; returns (results, outputs) as lz4_decompress_blocks.  codec: "uncompressed",
    "snappy", "gzip", "zstd" or "lz4_raw" (the column's CompressionCodec); an output is the pages' decoded bytes one after another
    (parquet_pages says where each begins).  verify_crc: check the CRC-32 of every page whose header carries one.
    output_lens=None: the sizes are asked for first (parquet_chunk_sizes; the input then crosses the link twice): a chunk the walk
    rejects gets the walk's code as its result and an empty output.  The footer's total_uncompressed_size is an upper bound on the
    decoded length: it always suffices as an output_len."""
    what, flags = _parquet_codec(codec), N.PARQUET_FLAG_VERIFY_CRC if verify_crc else 0
    run = lambda caps: _run(what, N.OP_DECOMPRESS, flags, chunks, caps, devices, out, N.PARQUET)
    if output_lens is not None:
        return run(output_lens)
    return _sizes_first(parquet_chunk_sizes(chunks, codec, devices), run)


def parquet_pages(chunks, devices=None):
    """the page tables of many Parquet column chunks held on the host: per chunk a (pages, 8) int64 array, or the walk's negative CJ_E_*
    code.  A row: page type; payload offset in the chunk; compressed_page_size; uncompressed_page_size; offset in the decoded chunk;
    num_values | num_rows << 32; encoding | def-level encoding << 8 | rep-level encoding << 16 | is_compressed << 24 | has_crc << 25;
    definition_levels_byte_length | repetition_levels_byte_length << 32."""
    import numpy as np

    def work(dev, idx):
        arrs = [np.frombuffer(chunks[i], dtype=np.uint8) for i in idx]          # borrowed, not copied
        k, L, h = len(arrs), N.lib(), _engine(dev).h
        ptrs = (_C.c_void_p * max(k, 1))(*[a.ctypes.data if a.size else None for a in arrs])
        lens = (_C.c_size_t * max(k, 1))(*[a.size for a in arrs])
        cnt = np.empty(k, np.int64)
        N.check(L.cj_parquet_pages_host(h, 0, k, ptrs, lens, None, None, cnt.ctypes.data))
        tabs = [np.empty((max(int(c), 0), 8), np.int64) for c in cnt]
        rows = (_C.c_void_p * max(k, 1))(*[t.ctypes.data for t in tabs])
        caps = (_C.c_size_t * max(k, 1))(*[len(t) for t in tabs])
        res = np.empty(k, np.int64)
        N.check(L.cj_parquet_pages_host(h, 0, k, ptrs, lens, rows, caps, res.ctypes.data))
        return ([t if r >= 0 else int(r) for t, r in zip(tabs, res)],)
    return _shard(devices, len(chunks), work)[0]


def parquet_decompress_chunks_device(inp, in_off, in_len, out, out_off, out_cap, codec, verify_crc=False, result=None, device=None, stream=None, sync=True):
    """Decode a device-resident batch of Parquet column chunks (arguments as lz4_decompress_frames_device; the call waits for the
    stream once, for the chunks' page counts)."""
    flags = N.PARQUET_FLAG_VERIFY_CRC if verify_crc else 0
    return _device_batch(N.PARQUET, _parquet_codec(codec), N.OP_DECOMPRESS, flags, inp, in_off, in_len, out, out_off, out_cap, result, device, stream, sync)


def parquet_chunk_sizes_device(inp, in_off, in_len, codec, result=None, device=None, stream=None, sync=True):
    """Decoded sizes of a device-resident batch of Parquet column chunks, as parquet_chunk_sizes; enqueue-only like lz4_block_sizes_device."""
    return _device_sizes(N.PARQUET, _parquet_codec(codec), 0, inp, in_off, in_len, result, device, stream, sync)


def parquet_pages_device(inp, in_off, in_len, rows=None, row_off=None, row_cap=None, result=None, device=None, stream=None, sync=True):
    """The page tables of a device-resident batch of Parquet column chunks.  rows=None: result[i] = chunk i's page count (or the walk's
    code).  Otherwise rows is a device buffer of 64-bit integers: chunk i's pages are written, eight words each as in parquet_pages, at
    rows[8 * row_off[i]:], row_cap[i] pages at most (more: -6, nothing written), and result[i] is the page count.  Enqueue-only with
    device-resident metadata, a result tensor and sync=False."""
    call = _DeviceCall(stream, sync)
    try:
        vin = call.buffer(inp)
        vrows = call.buffer(rows) if rows is not None else None
        eng = call.engine(device, vin)
        if vrows is not None and vrows.itemsize != 8:
            raise TypeError("cramjam_amd.batch: rows must hold 64-bit integers")
        p_in_off, p_in_len = call.meta(in_off, "in_off"), call.meta(in_len, "in_len")
        p_off = call.meta(row_off, "row_off") if vrows is not None else None
        p_cap = call.meta(row_cap, "row_cap") if vrows is not None else None
        p_res = call.result(result)
        N.check(N.lib().cj_parquet_pages_device(eng.h, 0, call.n, vin.ptr, p_in_off, p_in_len, vrows.ptr if vrows is not None else None, p_off, p_cap, p_res, stream))
        return call.finish(p_res, result)
    finally:
        call.close()


# ---- Parquet column chunks, written (cj_parquet_compress_* / cj_parquet_compress_bound) ----------------------------------
# The input of one entry is a DECODED chunk — what parquet_decompress_chunks gives — and its page table in parquet_pages' layout, so
# decode -> parquet_pages -> parquet_compress_chunks with another codec is Parquet-to-Parquet recompression.  The writer reads word 0
# (the type; its high half is V2's num_nulls, which parquet_pages leaves 0), 3, 5, 6 (the encodings; bit 25: write a crc) and 7.
# result[i] = the chunk's length or a negative CJ_E_* code: -73 an inconsistent table, -1 a chunk above 0x7E000000 bytes, the encoder's
# code of a V1 or dictionary page, -6 a chunk that does not fit its capacity; a chunk with a code writes nothing.
_PARQUET_ROW_CRC = 1 << 25


def parquet_compress_bound(codec, n, pages):
    """the capacity that suffices for a decoded chunk of n bytes in `pages` pages, however the pages cut it: pages * (57 + K) + n + g(n)
    (cramjam_hip.h); 0 above 0x7E000000 bytes.  No device."""
    return N.lib().cj_parquet_compress_bound(_parquet_codec(codec), n, pages)


def _parquet_table(t, write_crc):
    import numpy as np
    a = np.array(t, dtype=np.int64).reshape(-1, 8) if write_crc is not None else np.ascontiguousarray(np.asarray(t, dtype=np.int64).reshape(-1, 8))
    if write_crc is not None:
        a[:, 6] = (a[:, 6] | _PARQUET_ROW_CRC) if write_crc else (a[:, 6] & ~_PARQUET_ROW_CRC)
    return a


def parquet_compress_chunks(buffers, tables, codec, write_crc=None, devices=None, out=None):
    """write many Parquet column chunks, page-parallel: buffers[i] is a decoded chunk, tables[i] its (pages, 8) int64 page table as
    parquet_pages returns it; returns (results, chunks) as lz4_compress_blocks.  codec: as in parquet_decompress_chunks.  Per page a
    Thrift compact PageHeader (no Statistics), a V2 page's levels, and the values through the codec — a V2 page whose values do not
    shrink carries them raw with is_compressed = false.  write_crc: True / False sets / clears bit 25 of every row (a copy of the table)
    before the call, None leaves the rows' own bits.  out: as in lz4_decompress_blocks; it has to hold
    sum(parquet_compress_bound(codec, len(buffer), len(table))) bytes."""
    import numpy as np
    what, n = _parquet_codec(codec), len(buffers)
    if len(tables) != n:
        raise ValueError("cramjam_amd.batch: %d tables for %d buffers" % (len(tables), n))
    arrs = [np.frombuffer(b, dtype=np.uint8) for b in buffers]                  # borrowed, not copied
    tabs = [_parquet_table(t, write_crc) for t in tables]
    L = N.lib()
    caps = [L.cj_parquet_compress_bound(what, a.size, len(t)) for a, t in zip(arrs, tabs)]
    offsets, run = [], 0
    for c in caps:
        offsets.append(run); run += int(c)
    if out is None:
        dst = np.empty(run, np.uint8)
    else:
        dst = np.frombuffer(out, dtype=np.uint8)
        if dst.size < run:
            raise ValueError("cramjam_amd.batch: out holds %d bytes, the bounds need %d" % (dst.size, run))

    def work(dev, idx):
        k, h = len(idx), _engine(dev).h
        ptrs = (_C.c_void_p * max(k, 1))(*[arrs[i].ctypes.data if arrs[i].size else None for i in idx])
        lens = (_C.c_size_t * max(k, 1))(*[arrs[i].size for i in idx])
        rows = (_C.c_void_p * max(k, 1))(*[tabs[i].ctypes.data if len(tabs[i]) else None for i in idx])
        cnts = (_C.c_size_t * max(k, 1))(*[len(tabs[i]) for i in idx])
        outs = (_C.c_void_p * max(k, 1))(*[dst.ctypes.data + offsets[i] if caps[i] else None for i in idx])
        ocap = (_C.c_size_t * max(k, 1))(*[caps[i] for i in idx])
        res = np.empty(k, np.int64)
        N.check(L.cj_parquet_compress_host(h, what, 0, k, ptrs, lens, rows, cnts, outs, ocap, res.ctypes.data))
        return ([int(r) for r in res],)
    res, = _shard(devices, n, work)
    mv = memoryview(dst)
    views = [mv[offsets[i]:offsets[i] + max(res[i], 0)] for i in range(n)]
    return res, (views if out is not None else [bytes(v) for v in views])


def parquet_compress_chunks_device(inp, in_off, in_len, rows, row_off, row_cnt, out, out_off, out_cap, codec, result=None, device=None, stream=None, sync=True):
    """Write a device-resident batch of decoded chunks as Parquet column chunks (arguments as parquet_decompress_chunks_device; rows is
    a device buffer of 64-bit integers: chunk i's table is row_cnt[i] rows of eight words at rows[8 * row_off[i]:], as
    parquet_pages_device writes them).  The call waits for the stream once, for the chunks' plans; a capacity below
    parquet_compress_bound is allowed — a chunk that does not fit gets -6 and writes nothing."""
    call = _DeviceCall(stream, sync)
    try:
        vin, vrows, vout = call.buffer(inp), call.buffer(rows), call.buffer(out)
        eng = call.engine(device, vin, vout)
        if vrows.itemsize != 8:
            raise TypeError("cramjam_amd.batch: rows must hold 64-bit integers")
        i = (vin.ptr, call.meta(in_off, "in_off"), call.meta(in_len, "in_len"))
        t = (vrows.ptr, call.meta(row_off, "row_off"), call.meta(row_cnt, "row_cnt"))
        o = (vout.ptr, call.meta(out_off, "out_off"), call.meta(out_cap, "out_cap"))
        p_res = call.result(result)
        N.check(N.lib().cj_parquet_compress_device(eng.h, _parquet_codec(codec), 0, call.n, *i, *t, *o, p_res, stream))
        return call.finish(p_res, result)
    finally:
        call.close()
