"""Thin Python layer over the C ABI: pointer tables from torch tensors, workspace cache,
per-stage calls.  PyTorch is plumbing here (device memory + streams); the arithmetic is in
csrc/*.hip.  Nothing in this module falls back to PyTorch math.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _abi, _lib


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dev_f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def resolve_device(device: torch.device) -> torch.device:
    """``cuda`` without an index means the device that is current now, for good."""
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _readable_in_place(t: torch.Tensor, device: torch.device) -> bool:
    """True when a kernel on ``device`` can read ``t`` where it is: it lives there or in pinned host memory (a pageable host pointer
    would be a GPU page fault that aborts the process)."""
    return t.device == device or (t.device.type == "cpu" and t.is_pinned())


def _hip_device(device, who: str, cpu_path: str) -> torch.device:
    """The device a plan of the frame kernels runs on; ``cpu_path`` is what the error points a CPU caller to."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{who} runs on a HIP device (got {device}); {cpu_path} is the CPU path")
    return resolve_device(device)


def _in_place(name: str, t: torch.Tensor, dtype: torch.dtype, device: torch.device, count: Optional[int] = None) -> torch.Tensor:
    """``t`` as the contiguous flat tensor a kernel on ``device`` reads where it is: of ``dtype``, ``count`` values when given, on the
    device or in pinned host memory -- checked on the flat tensor, since the copy that flattening a strided host tensor makes is pageable."""
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if count is not None and t.numel() != count:
        raise ValueError(f"{name} must hold one value per frame ({count}), got {t.numel()}")
    flat = t.reshape(-1).contiguous()
    if not _readable_in_place(flat, device):
        raise ValueError(f"{name} must live on {device} or in pinned host memory (it is on {flat.device}, not pinned)")
    return flat


def config_coverage(cfg: _abi.AftConfig) -> Optional[str]:
    """None when the gfx950 kernels cover ``cfg``, else the library's reason (``aft_check_config``)."""
    lib = _lib.load()
    if lib.aft_check_config(C.byref(cfg)) == _abi.AFT_OK:
        return None
    return lib.aft_last_error().decode(errors="replace")


def conv_enhancer_covered(num_scs: int, num_symbols: int) -> bool:
    """True when the fused conv-stack kernel has a plan for this grid (row bands and, past what a band holds, column tiles)."""
    return _lib.load().aft_conv_enhancer_scratch_bytes(1, int(num_scs), int(num_symbols)) > 0


class HipEngine:
    """Owns an ``aft_config``, the weight pointer table and a workspace for one model.

    ``tensors`` maps reference ``state_dict`` keys to float32 CUDA
    tensors; the engine keeps references so the device pointers stay valid.
    """

    def __init__(self, cfg: _abi.AftConfig, tensors: Dict[str, torch.Tensor], lib=None):
        self.lib = lib if lib is not None else _lib.load()
        self.cfg = cfg
        self.device = next(iter(tensors.values())).device
        if self.device.type != "cuda":
            raise ValueError("HipEngine needs tensors on a HIP ('cuda') device")
        self._keep = {}
        for k, v in tensors.items():
            if not v.is_floating_point():
                continue
            if v.dtype != torch.float32 or not v.is_contiguous():
                raise ValueError(f"{k}: HIP path needs contiguous float32 (got {v.dtype})")
            self._keep[k] = v
        self.weights = _abi.make_weights(cfg, lambda k: self._keep[k].data_ptr(), pos_key=_abi.pos_key_of(self._keep))
        # the switch AFT_ENCODER_PATH=launches (A/B runs) overrides the automatic choice between the layer-by-layer launches and
        # the fused layer sequence (same output bits either way); `plane`: retired, runs the launches
        forced = _lib.get_switch("AFT_ENCODER_PATH")
        if forced:
            cfg.encoder_path = {"auto": _abi.AFT_ENCODER_AUTO, "launches": _abi.AFT_ENCODER_LAUNCHES,
                                "plane": _abi.AFT_ENCODER_PLANE}[forced]
        # scratch is PER STREAM: forwards in flight on different streams must not share the conv_enhanced / x / q / k / v^T
        # regions (nothing orders them against each other); each buffer is allocated with its stream current, so torch's
        # caching allocator re-uses it only in that stream's order
        self._ws: Dict[int, torch.Tensor] = {}
        self._ws_batch: Dict[int, int] = {}
        self.max_batch = int(self.lib.aft_max_batch(C.byref(cfg)))   # 32-bit buffer offsets: larger batches run in chunks
        # OPT-IN fragment-packed image of the encoder's GEMM weights (forward(cache_packed=True): for callers that know
        # their weights are constant, e.g. A/B tools); the default forward is stateless and re-packs inside the call
        lp = f"{_abi._TE}.transformer.layers."
        self._gemm_weights = [v for k, v in self._keep.items() if k.startswith(lp) and k.endswith(
            ("in_proj_weight", "out_proj.weight", "linear1.weight", "linear2.weight"))]
        self._packed: Dict[int, torch.Tensor] = {}
        self._packed_key: Dict[int, tuple] = {}

    MAX_STREAMS = 8      # scratch buffers kept (one per stream that ran a forward); the least recently used is dropped beyond that

    # -- helpers ---------------------------------------------------------------------------
    @property
    def tokens(self) -> int:
        return self.cfg.tokens

    def signature(self):
        return tuple(v.data_ptr() for v in self._keep.values())

    def workspace(self, batch: int) -> torch.Tensor:
        """The calling stream's scratch buffer (grown on demand)."""
        stream = self._stream()
        ws = self._ws.get(stream)
        if ws is not None:   # least-recently-used order: the entry in use moves to the end (eviction below drops the front)
            for table in (self._ws, self._ws_batch, self._packed, self._packed_key):
                if stream in table:
                    table[stream] = table.pop(stream)
        if ws is None or batch > self._ws_batch[stream]:
            # (with room for the fused layer sequence's two blocks behind the planned slices; the same size where it does not apply)
            nbytes = self.lib.aft_workspace_bytes_layer_fused(C.byref(self.cfg), batch)
            if nbytes == 0:
                _lib.check(self.lib.aft_forward_f32(C.byref(self.cfg), None, None, None, None, None, None, None, 0, batch, None))
                raise ValueError("unsupported configuration")
            if ws is None and len(self._ws) >= self.MAX_STREAMS:
                oldest = next(iter(self._ws))
                for table in (self._ws, self._ws_batch, self._packed, self._packed_key):
                    table.pop(oldest, None)
            with torch.cuda.device(self.device):
                ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws[stream], self._ws_batch[stream] = ws, batch
        return ws

    def _stream(self) -> int:
        return _lib.current_stream_ptr(self.device)

    def invalidate_packed(self) -> None:
        self._packed_key.clear()

    def packed_weights(self) -> torch.Tensor:
        """OPT-IN (cache_packed=True): this stream's packed image, re-built (5 us kernel on the current stream) when a GEMM
        weight's autograd version counter moved or after invalidate_packed().  Raw writes through ``.data`` / device
        pointers do NOT move the counters: a caller who makes them must call invalidate_packed() -- which is why the module
        surface does not use the cache."""
        stream = self._stream()
        key = (int(self.cfg.precision), tuple(t._version for t in self._gemm_weights))
        if self._packed_key.get(stream) != key:
            nbytes = self.lib.aft_packed_weights_bytes(C.byref(self.cfg))
            if stream not in self._packed:
                with torch.cuda.device(self.device):
                    self._packed[stream] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.aft_pack_weights_f32(C.byref(self.cfg), C.byref(self.weights), self._packed[stream].data_ptr(),
                                                     nbytes, stream))
            self._packed_key[stream] = key
        return self._packed[stream]

    # -- full forward ----------------------------------------------------------------------
    def forward(self, pilots: torch.Tensor, snr=None, ds=None, dop=None, out: Optional[torch.Tensor] = None,
                cache_packed: bool = False, pinned_inputs: bool = False) -> torch.Tensor:
        """pilots complex64 [B,Ps,Pt] -> complex64 [B,S,T] on the device, asynchronous on the current stream.  Any batch
        size: batches above ``max_batch`` (the ABI's 32-bit-offset limit) run as consecutive chunks, as the reference
        accepts any B (fortitran.py:145-182).  Default = aft_forward_f32, stateless: the encoder weights are re-laid
        into fragment order inside the call.  ``cache_packed``: use this engine's packed image instead
        (aft_forward_prepacked_f32; see packed_weights).  ``pinned_inputs``: pilots / conditions that live on the CPU are
        PINNED host tensors which the kernels read directly (device-addressable; the caller keeps them unchanged until the
        forward has run -- estimators._InputStager); without it every input must be on the engine's device."""
        c = self.cfg
        if pilots.dtype != torch.complex64:
            raise ValueError(f"pilot_symbols must be complex64, got {pilots.dtype}")
        if pilots.dim() != 3 or pilots.shape[1] * pilots.shape[2] != c.pilot_scs * c.pilot_symbols:
            raise ValueError(f"Expected pilot shape (B, {c.pilot_scs}, {c.pilot_symbols}), got {tuple(pilots.shape)}")
        B = pilots.shape[0]
        if pilots.device.type == "cpu" and not pinned_inputs:
            raise ValueError("pilot_symbols must be on the engine's device (or pinned, with pinned_inputs=True)")
        if pilots.device.type == "cpu" and not (_readable_in_place(pilots, self.device) and pilots.is_contiguous()):
            # a pageable (or silently re-copied non-contiguous) host pointer would be a GPU page fault that aborts the process
            raise ValueError("pinned_inputs=True needs contiguous pinned host tensors (pilot_symbols is not)")
        pil = torch.view_as_real(pilots.contiguous())
        metas = [None, None, None]
        if c.adaptive:
            if snr is None or ds is None or dop is None:
                raise ValueError("meta_data is required when channel adaptation is enabled")
            # host conditions are read in place only when they are pinned, contiguous float32; anything else is copied to the device
            metas = [m.reshape(-1) if (pinned_inputs and m.device.type == "cpu" and m.dtype == torch.float32 and m.is_contiguous()
                                       and _readable_in_place(m, self.device))
                     else _dev_f32(m.reshape(-1), self.device) for m in (snr, ds, dop)]
            if any(m.numel() != B for m in metas):
                raise ValueError("meta_data tensors must have one value per frame")
        if out is None:
            out = torch.empty((B, c.num_scs, c.num_symbols), dtype=torch.complex64, device=self.device)
        if B == 0:
            return out
        chunk = min(B, self.max_batch)
        ws = self.workspace(chunk)
        out_r = torch.view_as_real(out)
        packed = self.packed_weights() if cache_packed else None
        for lo in range(0, B, chunk):
            n = min(chunk, B - lo)
            m = [None if t is None else t[lo:lo + n].data_ptr() for t in metas]
            if packed is None:
                rc = self.lib.aft_forward_f32(C.byref(c), C.byref(self.weights), pil[lo:lo + n].data_ptr(), m[0], m[1], m[2],
                                              out_r[lo:lo + n].data_ptr(), ws.data_ptr(), ws.numel(), n, self._stream())
            else:
                rc = self.lib.aft_forward_prepacked_f32(C.byref(c), C.byref(self.weights), packed.data_ptr(),
                                                        pil[lo:lo + n].data_ptr(), m[0], m[1], m[2],
                                                        out_r[lo:lo + n].data_ptr(), ws.data_ptr(), ws.numel(), n,
                                                        self._stream())
            _lib.check(rc)
        return out

    def forward_region(self, name: str, batch: int) -> torch.Tensor:
        """What the last ``forward`` of ``batch`` frames on the current stream left in the workspace (``aft_workspace_region``):
        'conv_enhanced' f32 [2B,S,T], 'tokens6' f32 [B,tokens,6], 'enc_out' f32 [2B,tokens,8|16] -- the production kernels'
        intermediates, for known-answer tests.  A copy, valid whatever runs next."""
        c = self.cfg
        ws = self._ws[self._stream()]
        # the forward may have run as several lanes (contiguous shares of the batch, each with its own slice of the workspace)
        lanes, frames, bases = C.c_int(), (C.c_int * 4)(), (C.c_size_t * 4)()
        _lib.check(self.lib.aft_workspace_lanes(C.byref(c), batch, C.byref(lanes), frames, bases))
        parts = []
        for i in range(lanes.value):
            off, size = C.c_size_t(), C.c_size_t()
            _lib.check(self.lib.aft_workspace_region(C.byref(c), frames[i], _abi.REGION_IDS[name], C.byref(off), C.byref(size)))
            flat = ws[bases[i] + off.value:bases[i] + off.value + size.value].view(torch.float32).clone()
            shape = {"conv_enhanced": (2 * frames[i], c.num_scs, c.num_symbols), "tokens6": (frames[i], self.tokens, 6),
                     "enc_out": (2 * frames[i], self.tokens, -1)}[name]
            parts.append(flat.view(*shape))
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)

    # -- per-stage entry points (tests) ----------------------------------------------------
    def stage_upsample(self, pilots: torch.Tensor) -> torch.Tensor:
        B = pilots.shape[0]
        out = torch.empty((2 * B, self.cfg.num_scs, self.cfg.num_symbols), dtype=torch.float32, device=self.device)
        pil = torch.view_as_real(pilots.contiguous())
        _lib.check(self.lib.aft_stage_upsample_f32(C.byref(self.cfg), C.byref(self.weights), pil.data_ptr(),
                                                   out.data_ptr(), B, self._stream()))
        return out

    def stage_adapter(self, snr, ds, dop) -> torch.Tensor:
        m = [_dev_f32(t.reshape(-1), self.device) for t in (snr, ds, dop)]
        B = m[0].numel()
        out = torch.empty((B, self.tokens, 6), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.aft_stage_adapter_f32(C.byref(self.cfg), C.byref(self.weights), m[0].data_ptr(),
                                                  m[1].data_ptr(), m[2].data_ptr(), out.data_ptr(), B, self._stream()))
        return out

    def stage_embed(self, conv_enhanced: torch.Tensor, tokens6: Optional[torch.Tensor]) -> torch.Tensor:
        B = conv_enhanced.shape[0] // 2
        x = torch.empty((2 * B, self.tokens, self.cfg.model_dim), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.aft_stage_embed_f32(C.byref(self.cfg), C.byref(self.weights), conv_enhanced.data_ptr(),
                                                _ptr(tokens6), x.data_ptr(), B, self._stream()))
        return x

    def stage_encoder_layer(self, layer: int, x: torch.Tensor) -> torch.Tensor:
        """x float32 [2B, tokens, d] -> new tensor, one post-LN encoder layer."""
        y = x.contiguous().clone()
        B = y.shape[0] // 2
        ws = self.workspace(B)
        _lib.check(self.lib.aft_stage_encoder_layer_f32(C.byref(self.cfg), C.byref(self.weights), layer, y.data_ptr(),
                                                        ws.data_ptr(), ws.numel(), B, self._stream()))
        return y

    def stage_tail(self, x: torch.Tensor, conv_enhanced: torch.Tensor) -> torch.Tensor:
        B = conv_enhanced.shape[0] // 2
        out = torch.empty((B, self.cfg.num_scs, self.cfg.num_symbols), dtype=torch.complex64, device=self.device)
        x, conv_enhanced = x.contiguous(), conv_enhanced.contiguous()    # keep both alive across the launch
        _lib.check(self.lib.aft_stage_tail_f32(C.byref(self.cfg), C.byref(self.weights), x.data_ptr(),
                                               conv_enhanced.data_ptr(),
                                               torch.view_as_real(out).data_ptr(), B, self._stream()))
        return out


def fill_lds(value: float, device="cuda:0") -> None:
    """Test hook (aft_debug_fill_lds_f32): every CU's LDS filled with ``value`` on the current stream -- what the next kernels find in
    their LDS at start."""
    dev = torch.device(device)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().aft_debug_fill_lds_f32(C.c_float(value), _lib.current_stream_ptr(dev)))


def peek_lds(workgroups: int = 1024, n: int = 1024, device="cuda:0") -> torch.Tensor:
    """Test hook (aft_debug_peek_lds_f32): what ``workgroups`` fresh workgroups find in the first ``n`` floats of their LDS."""
    dev = torch.device(device)
    with torch.cuda.device(dev):
        out = torch.empty((workgroups, n), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().aft_debug_peek_lds_f32(out.data_ptr(), workgroups, n, _lib.current_stream_ptr(dev)))
    return out


def profile_kernel(eng: HipEngine, which: str, batch: int, reps: int, io: Optional[torch.Tensor] = None) -> None:
    """Enqueue ``reps`` launches of one kernel class on the current stream (bench.py roofline leg)."""
    ws = eng.workspace(batch)
    ptr = None if io is None else (torch.view_as_real(io) if io.is_complex() else io).data_ptr()
    _lib.check(eng.lib.aft_profile_kernel_f32(C.byref(eng.cfg), C.byref(eng.weights), _abi.KERNEL_IDS[which], ptr,
                                              ws.data_ptr(), ws.numel(), batch, reps, eng._stream()))


def engine_from_numpy(cfg: _abi.AftConfig, state: Dict[str, np.ndarray], device="cuda:0", lib=None) -> HipEngine:
    """Upload a numpy state_dict (e.g. from ``synth.make_state_dict``) and build an engine."""
    dev = torch.device(device)
    tensors = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in state.items()}
    return HipEngine(cfg, tensors, lib=lib)


def linear_forward(weight: torch.Tensor, bias: Optional[torch.Tensor], pilots: torch.Tensor, ofdm_size) -> torch.Tensor:
    """LinearEstimator on the HIP device, plane-wise on complex64 pilots [B,Ps,Pt]."""
    lib = _lib.load()
    if pilots.dtype != torch.complex64:
        raise ValueError("pilots must be complex64")
    B = pilots.shape[0]
    out_f, in_f = weight.shape
    if pilots[0].numel() != in_f or ofdm_size[0] * ofdm_size[1] != out_f:
        raise ValueError("shape mismatch between pilots / weight / ofdm_size")
    pil = torch.view_as_real(pilots.contiguous())
    weight = weight.contiguous()
    out = torch.empty((B, ofdm_size[0], ofdm_size[1]), dtype=torch.complex64, device=pilots.device)
    _lib.check(lib.aft_linear_forward_f32(weight.data_ptr(), _ptr(bias), pil.data_ptr(),
                                          torch.view_as_real(out).data_ptr(), B, in_f, out_f,
                                          _lib.current_stream_ptr(pilots.device)))
    return out


def mse_sum(est: torch.Tensor, ref: torch.Tensor, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Accumulate sum |est-ref|^2 (float64 device scalar) without a host sync."""
    lib = _lib.load()
    if est.dtype != torch.complex64 or ref.dtype != torch.complex64 or est.shape != ref.shape:
        raise ValueError("est/ref must be complex64 tensors of equal shape")
    if acc is None:
        acc = torch.zeros(1, dtype=torch.float64, device=est.device)
    e, r = torch.view_as_real(est.contiguous()), torch.view_as_real(ref.contiguous())
    _lib.check(lib.aft_mse_partial_f32(e.data_ptr(), r.data_ptr(), acc.data_ptr(), est.numel(),
                                       _lib.current_stream_ptr(est.device)))
    return acc


def pilot_gather(hzero_ls: torch.Tensor, pilot_size, return_counts: bool = False):
    """Sparse LS grid complex64 [B,S,T] (zeros off the pilot positions) -> pilots complex64
    [B,Ps,Pt], the non-zero entries in row-major order (reference dataset.py:116-139).  Raises the
    reference's ValueError when a frame does not hold exactly Ps*Pt non-zero entries -- which costs one
    host sync; ``return_counts=True`` returns ``(pilots, counts int32 [B])`` instead and leaves the check
    (``check_pilot_counts``) to the caller, who can run it off the critical path (ingest.PackedLoader)."""
    lib = _lib.load()
    if hzero_ls.dtype != torch.complex64 or hzero_ls.dim() != 3:
        raise ValueError("hzero_ls must be complex64 [B, S, T]")
    B, n = hzero_ls.shape[0], hzero_ls.shape[1] * hzero_ls.shape[2]
    expected = int(pilot_size[0]) * int(pilot_size[1])
    src = torch.view_as_real(hzero_ls.contiguous())
    out = torch.empty((B, pilot_size[0], pilot_size[1]), dtype=torch.complex64, device=hzero_ls.device)   # the kernel writes every slot
    counts = torch.empty(B, dtype=torch.int32, device=hzero_ls.device)
    _lib.check(lib.aft_pilot_gather_f32(src.data_ptr(), torch.view_as_real(out).data_ptr(), counts.data_ptr(), B, n,
                                        expected, _lib.current_stream_ptr(hzero_ls.device)))
    if return_counts:
        return out, counts
    check_pilot_counts(counts, expected)
    return out


def check_pilot_counts(counts: torch.Tensor, expected: int, first_frame: int = 0) -> None:
    """The reference's "Expected 24 pilot values, got 25" error (dataset.py:133-139) from the kernel's per-frame counts
    (a device or host int32 tensor)."""
    bad = (counts != expected).nonzero()
    if bad.numel():
        i = int(bad[0])
        raise ValueError(f"Expected {expected} pilot values, got {int(counts[i])} (frame {first_frame + i})")


def frame_gather(ideal_all: torch.Tensor, pilots_all: torch.Tensor, index: torch.Tensor, lib=None):
    """Frames ``index`` (int64 [b], on the HIP device) of two resident complex64 arrays ``ideal_all [n, ...]`` and ``pilots_all [n, ...]``
    -> ``(ideal [b, ...], pilots [b, ...], flags int32 [b])`` on the index's device, in ONE launch on its current stream
    (``aft_frame_gather_f32``).  Either array lives on that device or in pinned host memory (read in place over the link); both must be
    contiguous.  An entry outside ``[0, n)`` gives a zero frame and ``flags == 1`` there; the call itself never synchronises, so a
    caller that did not make the indices itself checks ``flags`` when it can afford to.  ``lib``: another build of the library
    (``_lib.load_path``), for the tests that compare builds."""
    lib = lib or _lib.load()
    if index.dtype != torch.int64 or index.dim() != 1 or index.device.type != "cuda" or not index.is_contiguous() or index.numel() < 1:
        raise ValueError("index must be a contiguous, non-empty int64 vector on the HIP device")
    dev = index.device
    for name, t in (("ideal_all", ideal_all), ("pilots_all", pilots_all)):
        if t.dtype != torch.complex64 or t.dim() < 2 or not t.is_contiguous() or t.shape[0] < 1 or t[0].numel() < 1:
            raise ValueError(f"{name} must be a contiguous complex64 array [n, ...] with n >= 1")
        _in_place(name, t, torch.complex64, dev)
    if ideal_all.shape[0] != pilots_all.shape[0]:
        raise ValueError(f"ideal_all holds {ideal_all.shape[0]} frames, pilots_all {pilots_all.shape[0]}")
    plan = FrameGatherPlan(ideal_all, pilots_all, dev)
    with torch.cuda.device(dev):
        return plan(index, lib)


class FrameGatherPlan:
    """Two resident arrays that ``frame_gather`` has accepted, with everything a launch needs taken from them ONCE: a caller that
    gathers from the same arrays for every batch (ingest.ResidentLoader) pays two ``torch.empty`` (three with the flags), one ``ctypes``
    call and nothing else per batch.  ``plan(index)`` trusts its caller: ``index`` is a contiguous, non-empty int64 vector on the
    plan's device and that device is the current one."""

    def __init__(self, ideal_all: torch.Tensor, pilots_all: torch.Tensor, device: torch.device) -> None:
        self.arrays = (ideal_all, pilots_all)                   # kept alive with the plan
        self.device = device
        self.src = (ideal_all.data_ptr(), pilots_all.data_ptr())
        self.n = ideal_all.shape[0]
        self.tails = (tuple(ideal_all.shape[1:]), tuple(pilots_all.shape[1:]))
        self.elems = (ideal_all[0].numel(), pilots_all[0].numel())

    def __call__(self, index: torch.Tensor, lib=None):
        lib = lib or _lib.load()
        b, dev = index.shape[0], self.device
        ideal = torch.empty((b, *self.tails[0]), dtype=torch.complex64, device=dev)      # the kernel writes every element
        pilots = torch.empty((b, *self.tails[1]), dtype=torch.complex64, device=dev)
        flags = torch.empty(b, dtype=torch.int32, device=dev)
        _lib.check(lib.aft_frame_gather_f32(self.src[0], self.src[1], index.data_ptr(), ideal.data_ptr(), pilots.data_ptr(),
                                            flags.data_ptr(), b, self.n, self.elems[0], self.elems[1], _lib.current_stream_ptr(dev)))
        return ideal, pilots, flags


class ChannelSimPlan:
    """A channel-simulator configuration (``chansim.ChannelSimConfig``) that has been turned into the ``aft_chansim`` struct ONCE.
    ``plan(seed, base, start, stride, modulo, batch)`` -> ``(ideal complex64 [batch,S,T], pilots complex64 [batch,Ps,Pt], meta float32
    [batch,3])`` on the plan's device: three ``torch.empty``, one ``ctypes`` call, one launch (``aft_channel_sim_f32``) on the current
    stream of that device, no upload and no synchronisation.  Output frame b is global frame ``base + (start + b * stride) % modulo``.
    With a grouped configuration (``cfg.antennas``, G = R N frames per group) the launch is ``aft_channel_sim_group_f32``, the four
    position arguments count GROUPS -- output frame b is member ``b % G`` of group ``base + (start + (b // G) * stride) % modulo`` --
    and ``batch``, still in frames, is a multiple of G; the packed ``mix`` is host memory the plan keeps.
    With slot sequences (``cfg.slots`` = K > 1) the launch is ``aft_channel_sim_seq_f32``, the four position arguments count SEQUENCES
    of ``K G`` frames -- output frame b is member ``b % G`` of slot ``(b // G) % K`` of sequence ``base + (start + (b // (K G)) * stride)
    % modulo`` -- and ``batch`` is a multiple of ``K G``.  With ``slots = 1`` the launches are the ones above.
    The plan trusts its caller in one thing only: its device is the current one."""

    def __init__(self, cfg, device: torch.device) -> None:
        self.device = _hip_device(device, "ChannelSimPlan", "chansim.simulate_frames_host")
        self.cfg = cfg
        self.sim = cfg.to_struct()                              # validated by the config itself; the entry point checks again
        self.grid, self.pilot = tuple(cfg.ofdm), tuple(cfg.pilot)
        self.antennas, self.group = tuple(cfg.antennas), cfg.group
        self.slots, self.slot_symbols = cfg.slots, cfg.slot_symbols
        self.mix = pack_mix(cfg.mix()) if self.group > 1 or self.slots > 1 else None

    def __call__(self, seed: int, base: int, start: int, stride: int, modulo: int, batch: int, lib=None):
        lib = lib or _lib.load()
        dev = self.device
        ideal = torch.empty((batch, *self.grid), dtype=torch.complex64, device=dev)      # the kernel writes every element
        pilots = torch.empty((batch, *self.pilot), dtype=torch.complex64, device=dev)
        meta = torch.empty((batch, 3), dtype=torch.float32, device=dev)
        if self.slots > 1:
            _lib.check(lib.aft_channel_sim_seq_f32(self.sim, *self.antennas, self.mix.ctypes.data, self.slots, self.slot_symbols,
                                                   seed & 0xFFFFFFFFFFFFFFFF, base, start, stride, modulo, batch, ideal.data_ptr(),
                                                   pilots.data_ptr(), meta.data_ptr(), _lib.current_stream_ptr(dev)), lib)
            return ideal, pilots, meta
        if self.group > 1:
            _lib.check(lib.aft_channel_sim_group_f32(self.sim, *self.antennas, self.mix.ctypes.data, seed & 0xFFFFFFFFFFFFFFFF, base, start,
                                                     stride, modulo, batch, ideal.data_ptr(), pilots.data_ptr(), meta.data_ptr(),
                                                     _lib.current_stream_ptr(dev)), lib)
            return ideal, pilots, meta
        _lib.check(lib.aft_channel_sim_f32(self.sim, seed & 0xFFFFFFFFFFFFFFFF, base, start, stride, modulo, batch, ideal.data_ptr(),
                                           pilots.data_ptr(), meta.data_ptr(), _lib.current_stream_ptr(dev)), lib)
        return ideal, pilots, meta


def pack_mix(mix) -> np.ndarray:
    """The lower triangle of a complex ``[G, G]`` mixing matrix as ``aft_channel_sim_group_f32`` reads it: float32, row a's
    ``L[a][0 .. a]`` as (re, im) pairs at float offset ``a (a + 1)``."""
    m = np.asarray(mix, dtype=np.complex64)
    rows, cols = np.tril_indices(m.shape[0])                    # row-major over the lower triangle
    return np.ascontiguousarray(m[rows, cols]).view(np.float32)


class LmmsePlan:
    """The LMMSE baseline (``lmmse.LmmseTables``) turned into the ``aft_lmmse`` struct and its float32 table image on the device ONCE.
    ``plan(pilots, snr, ds, dop)`` -> ``est complex64 [batch,S,T]`` on the plan's device: one ``torch.empty``, one ``ctypes`` call, one
    launch (``aft_lmmse_f32``) on the current stream of that device, no synchronisation.  ``pilots`` complex64 ``[batch,Ps,Pt]`` and the
    three float32 conditions (``batch`` values each, any shape) live on the plan's device or in pinned host memory, which the kernel
    reads in place; a condition that ``assume`` pins may be None.  ``image``: the table image when the caller already holds it on
    the device (``lmmse.LmmseEstimator``'s buffer).  The plan trusts its caller in one thing only: its device is the current one."""

    def __init__(self, cfg, device: torch.device, assume=None, image: Optional[torch.Tensor] = None) -> None:
        from .lmmse import LmmseTables
        self.device = _hip_device(device, "LmmsePlan", "lmmse.lmmse_estimate_host")
        self.tables = cfg if isinstance(cfg, LmmseTables) else LmmseTables(cfg)
        self.plan = self.tables.to_struct(assume)
        self.fixed = (self.plan.fixed_snr, self.plan.fixed_ds, self.plan.fixed_dop)
        self.grid, self.pilot = tuple(self.tables.cfg.ofdm), tuple(self.tables.cfg.pilot)
        if image is None:
            image = torch.from_numpy(self._host_image()).to(self.device)
        floats = self._image_floats(_lib.load())
        if image.dtype != torch.float32 or image.device != self.device or not image.is_contiguous() or image.numel() != floats:
            raise ValueError(f"the table image must be {floats} contiguous float32 values on {self.device} (got {image.numel()} "
                             f"{image.dtype} on {image.device})")
        self.image = image

    def __call__(self, pilots: torch.Tensor, snr=None, ds=None, dop=None, lib=None) -> torch.Tensor:
        lib = lib or _lib.load()
        if pilots.dim() != 3 or tuple(pilots.shape[1:]) != self.pilot or pilots.shape[0] < 1:
            raise ValueError(f"Expected pilot shape (B >= 1, {self.pilot[0]}, {self.pilot[1]}), got {tuple(pilots.shape)}")
        batch = pilots.shape[0]
        pil = _in_place("pilots", pilots, torch.complex64, self.device)
        conds = []
        for name, c, fixed in zip(("snr", "ds", "dop"), (snr, ds, dop), self.fixed):
            if c is None:
                if fixed < 0:
                    raise ValueError(f"{name} is required: assume does not pin it")
                conds.append(None)
                continue
            conds.append(_in_place(name, c, torch.float32, self.device, batch))
        est = torch.empty((batch, *self.grid), dtype=torch.complex64, device=self.device)   # the kernel writes every element
        _lib.check(self._launch(lib, pil.data_ptr(), [_ptr(c) for c in conds], est.data_ptr(), batch), lib)
        return est

    def _host_image(self) -> np.ndarray:
        return self.tables.image()

    def _image_floats(self, lib) -> int:
        return lib.aft_lmmse_table_floats(C.byref(self.plan))

    def _launch(self, lib, pilots: int, conds, est: int, batch: int) -> int:
        return lib.aft_lmmse_f32(C.byref(self.plan), self.image.data_ptr(), pilots, *conds, est, batch, _lib.current_stream_ptr(self.device))


class LmmseSeqPlan(LmmsePlan):
    """``LmmsePlan`` for the multi-slot estimator (``lmmse.LmmseTables(cfg, window, horizon)``): the image is ``seq_image()`` and
    ``plan(pilots, snr, ds, dop)`` is one launch of ``aft_lmmse_seq_f32`` over a batch of WHOLE sequences in order (``batch`` a multiple of
    ``slots * group``; the entry point refuses anything else).  Everything else is ``LmmsePlan``'s: inputs on the device or in pinned
    host memory, None for a condition that ``assume`` pins, ``lib=`` for another build of the library."""

    def __init__(self, cfg, device: torch.device, assume=None, image: Optional[torch.Tensor] = None) -> None:
        from .lmmse import LmmseTables
        tables = cfg if isinstance(cfg, LmmseTables) else LmmseTables(cfg)
        self.group, self.slots = tables.cfg.group, tables.cfg.slots
        self.window, self.horizon = tables.window, tables.horizon
        super().__init__(tables, device, assume=assume, image=image)

    def _host_image(self) -> np.ndarray:
        return self.tables.seq_image()

    def _image_floats(self, lib) -> int:
        return lib.aft_lmmse_seq_table_floats(C.byref(self.plan), self.window)

    def _launch(self, lib, pilots: int, conds, est: int, batch: int) -> int:
        return lib.aft_lmmse_seq_f32(C.byref(self.plan), self.group, self.slots, self.window, self.horizon, self.image.data_ptr(), pilots,
                                     *conds, est, batch, _lib.current_stream_ptr(self.device))


class LmmseGridPlan:
    """The full-grid smoother (``lmmse.lmmse_grid_host`` is the definition) planned ONCE: the ``aft_lmmse`` struct with
    ``noise_var = float32(noise_scale * sigma2)`` and the float32 grid image (``LmmseTables.grid().image()``) on the device.
    ``plan(z, snr, ds, dop)`` -> ``est complex64 [batch,S,T]`` on the plan's device from the observations ``z complex64 [batch,S,T]``
    (device memory): one ``torch.empty``, one ``ctypes`` call, one launch (``aft_lmmse_grid_f32``) on the current stream, no
    synchronisation.  The three float32 conditions as ``LmmsePlan``'s.  A grid with more than 32 symbols is refused here, as by the
    entry point.  The plan trusts its caller in one thing only: its device is the current one."""

    def __init__(self, cfg, device: torch.device, assume=None, noise_scale: float = 1.0, image: Optional[torch.Tensor] = None) -> None:
        from .lmmse import LmmseTables
        self.device = _hip_device(device, "LmmseGridPlan", "lmmse.lmmse_grid_host")
        self.tables = cfg if isinstance(cfg, LmmseTables) else LmmseTables(cfg)
        grid = self.tables.grid()                               # refuses T > 32 with the message that says so
        self.kf, self.noise_scale = grid.kf, float(noise_scale)
        self.plan = grid.to_struct(assume, noise_scale)
        self.fixed = (self.plan.fixed_snr, self.plan.fixed_ds, self.plan.fixed_dop)
        self.grid = tuple(self.tables.cfg.ofdm)
        S, T = self.grid
        floats = self.plan.n_ds * (4 * S * self.kf + self.kf + (self.kf & 1)) + self.plan.n_dop * (2 * T * T + T)
        if image is None:
            image = torch.from_numpy(grid.image()).to(self.device)
        if image.dtype != torch.float32 or image.device != self.device or not image.is_contiguous() or image.numel() != floats:
            raise ValueError(f"the grid image must be {floats} contiguous float32 values on {self.device} (got {image.numel()} "
                             f"{image.dtype} on {image.device})")
        self.image = image

    def __call__(self, z: torch.Tensor, snr=None, ds=None, dop=None, lib=None) -> torch.Tensor:
        lib = lib or _lib.load()
        if z.dim() != 3 or tuple(z.shape[1:]) != self.grid or z.shape[0] < 1:
            raise ValueError(f"Expected observations of shape (B >= 1, {self.grid[0]}, {self.grid[1]}), got {tuple(z.shape)}")
        if z.dtype != torch.complex64 or z.device != self.device:
            raise ValueError(f"z must be complex64 on {self.device}, got {z.dtype} on {z.device}")
        batch = z.shape[0]
        z = z.contiguous()
        conds = []
        for name, c, fixed in zip(("snr", "ds", "dop"), (snr, ds, dop), self.fixed):
            if c is None:
                if fixed < 0:
                    raise ValueError(f"{name} is required: assume does not pin it")
                conds.append(None)
                continue
            conds.append(_in_place(name, c, torch.float32, self.device, batch))
        est = torch.empty((batch, *self.grid), dtype=torch.complex64, device=self.device)   # the kernel writes every element
        _lib.check(lib.aft_lmmse_grid_f32(C.byref(self.plan), self.kf, self.image.data_ptr(), z.data_ptr(), *[_ptr(c) for c in conds],
                                          est.data_ptr(), batch, _lib.current_stream_ptr(self.device)), lib)
        return est


class LmmseClassifyPlan:
    """The design point from the pilots (``lmmse.lmmse_classify_host`` is the definition) planned ONCE: the ``aft_lmmse`` struct, the
    estimator's own float32 image (``seq_image()`` with a window, ``image()`` without) and the log-determinant table
    (``LmmseTables.classify_image()``) on the device.  ``plan(pilots, scores=False)`` -> ``(idx int32 [batch,3], snr, ds, dop float32
    [batch][, scores float32 [units, n_snr n_ds n_dop]])`` on the plan's device: one ``torch.empty`` per output, one ``ctypes`` call, one
    launch (``aft_lmmse_classify_f32``) on the current stream of that device, no synchronisation.  ``pilots`` complex64
    ``[batch,Ps,Pt]`` live on the plan's device or in pinned host memory; ``batch`` is whole sequences (with single-slot tables: whole
    groups when pooling, anything otherwise).  ``pool``: a group of frames decides together (units = batch / group), else every frame
    alone.  ``image`` / ``logdet``: the tables when the caller already holds them on the device.  ``snr``, ``ds`` and ``dop`` are what
    ``LmmseSeqPlan`` / ``LmmsePlan`` of the same tables take as conditions.  The plan trusts its caller in one thing only: its device
    is the current one."""

    def __init__(self, cfg, device: torch.device, assume=None, pool: bool = True, image: Optional[torch.Tensor] = None,
                 logdet: Optional[torch.Tensor] = None) -> None:
        from .lmmse import LmmseTables
        self.device = _hip_device(device, "LmmseClassifyPlan", "lmmse.lmmse_classify_host")
        self.tables = tb = cfg if isinstance(cfg, LmmseTables) else LmmseTables(cfg)
        self.plan = tb.to_struct(assume)
        self.fixed = (self.plan.fixed_snr, self.plan.fixed_ds, self.plan.fixed_dop)
        self.pilot, self.pool = tuple(tb.cfg.pilot), bool(pool)
        self.window, self.horizon = tb.window, tb.horizon
        self.slots = tb.cfg.slots if tb.multi_slot else 1                       # single-slot tables look at no other slot ...
        self.group = tb.cfg.group if (tb.multi_slot or self.pool) else 1        # ... and a frame that decides alone at no other member
        self.candidates = self.plan.n_snr * self.plan.n_ds * self.plan.n_dop
        lib = _lib.load()
        if image is None:
            image = torch.from_numpy(tb.seq_image() if tb.multi_slot else tb.image()).to(self.device)
        if logdet is None:
            logdet = torch.from_numpy(tb.classify_image()).to(self.device)
        for name, t, floats in (("table image", image, lib.aft_lmmse_seq_table_floats(C.byref(self.plan), self.window)),
                                ("log-determinant table", logdet, lib.aft_lmmse_classify_table_floats(C.byref(self.plan), self.window))):
            if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or t.numel() != floats:
                raise ValueError(f"the {name} must be {floats} contiguous float32 values on {self.device} (got {t.numel()} {t.dtype} on "
                                 f"{t.device})")
        self.image, self.logdet = image, logdet

    def __call__(self, pilots: torch.Tensor, scores: bool = False, lib=None):
        lib = lib or _lib.load()
        if pilots.dim() != 3 or tuple(pilots.shape[1:]) != self.pilot or pilots.shape[0] < 1:
            raise ValueError(f"Expected pilot shape (B >= 1, {self.pilot[0]}, {self.pilot[1]}), got {tuple(pilots.shape)}")
        batch = pilots.shape[0]
        pil = _in_place("pilots", pilots, torch.complex64, self.device)
        idx = torch.empty((batch, 3), dtype=torch.int32, device=self.device)    # the kernel writes every element of all of them
        snr, ds, dop = (torch.empty((batch,), dtype=torch.float32, device=self.device) for _ in range(3))
        units = batch // self.group if self.pool else batch
        sc = torch.empty((units, self.candidates), dtype=torch.float32, device=self.device) if scores else None
        _lib.check(lib.aft_lmmse_classify_f32(C.byref(self.plan), self.group, self.slots, self.window, self.horizon, int(self.pool),
                                              self.image.data_ptr(), self.logdet.data_ptr(), pil.data_ptr(), idx.data_ptr(), snr.data_ptr(),
                                              ds.data_ptr(), dop.data_ptr(), _ptr(sc), batch, _lib.current_stream_ptr(self.device)), lib)
        return (idx, snr, ds, dop, sc) if scores else (idx, snr, ds, dop)


class LinkPlan:
    """A link configuration (``linksim.LinkConfig``) turned into the ``aft_link`` struct ONCE.  ``plan(ideal, est, keys, sigma)`` ->
    ``counts int32 [batch, 2]`` = (bit errors, symbol errors) per frame on the plan's device: one ``torch.empty``, one ``ctypes`` call,
    one launch (``aft_link_errors_f32``) on the current stream of that device, no synchronisation.  ``ideal`` / ``est`` complex64
    ``[batch,S,T]`` live on the plan's device; ``keys`` (int64, the 64-bit keys' bits) and ``sigma`` (float32), ``batch`` values each,
    live there or in pinned host memory, which the kernel reads in place.  The plan trusts its caller in one thing only: its device
    is the current one."""
    cpu_path = "linksim.link_errors_host"
    pairs = False                                               # True: a group is branches * 2 frames and yields one row (LinkAlamoutiPlan)
    n_sub = None                                                # an integer: the launch also writes pmi int32 [rows, n_sub] (LinkPrecodedPlan)
    n_stats = None                                              # an integer: the launch also writes stats int32 [groups, n_stats] (LinkSicPlan)
    slots, delay = 1, 0                                         # slots > 1: sequences of `slots` groups, feedback `delay` slots old (LinkPrecodedPlan)

    def __init__(self, cfg, device: torch.device) -> None:
        from .linksim import LinkConfig
        if not isinstance(cfg, LinkConfig):
            raise ValueError(f"{type(self).__name__} needs a linksim.LinkConfig (got {type(cfg).__name__})")
        self.device = _hip_device(device, type(self).__name__, self.cpu_path)
        self.cfg = cfg
        self.link = cfg.to_struct()                             # validated by the config itself; the entry point checks again
        self.grid = tuple(cfg.sim.ofdm)

    def _checked(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor):
        """The four operands every launch on this link takes, checked: ``(batch, ideal, est, keys, sigma)``."""
        if ideal.dim() != 3 or tuple(ideal.shape[1:]) != self.grid or ideal.shape[0] < 1:
            raise ValueError(f"Expected ideal shape (B >= 1, {self.grid[0]}, {self.grid[1]}), got {tuple(ideal.shape)}")
        batch = ideal.shape[0]
        if est.shape != ideal.shape:
            raise ValueError(f"est must have ideal's shape {tuple(ideal.shape)}, got {tuple(est.shape)}")
        for name, t in (("ideal", ideal), ("est", est)):
            if t.dtype != torch.complex64:
                raise ValueError(f"{name} must be complex64, got {t.dtype}")
            if t.device != self.device:
                raise ValueError(f"{name} must live on {self.device} (it is on {t.device})")
        return (batch, ideal.contiguous(), est.contiguous(),   # held by the caller until after the launch is enqueued
                _in_place("keys", keys, torch.int64, self.device, batch), _in_place("sigma", sigma, torch.float32, self.device, batch))

    def _checked_factors(self, factors: torch.Tensor) -> torch.Tensor:
        """The factors of a soft launch, checked: float32, 1 .. 8 values, on the plan's device or in pinned host memory."""
        if not torch.is_tensor(factors) or not 1 <= factors.numel() <= 8:
            raise ValueError(f"factors must hold between 1 and 8 values, got {factors.numel() if torch.is_tensor(factors) else factors!r}")
        return _in_place("factors", factors, torch.float32, self.device, factors.numel())

    def _grouped(self, entry: str, ideal, est, keys, sigma, rho, per_group, factors, want_llr: bool, lib):
        """What the grouped front ends (``LinkMrcPlan``, ``LinkSmPlan``, ``LinkJointPlan``, ``LinkSicPlan``) share.  ``self.group`` is the group's
        width, ``(branches,)`` or ``(branches, streams)``, passed to ``entry`` as it stands; ``per_group`` names the float32 operands
        with one value per group, in the entry point's order.  Returns ``(counts, loss, llr)`` for ``groups * streams`` rows.
        ``LinkAlamoutiPlan`` sets ``self.pairs``: its group is ``branches * 2`` frames that yield ONE row, and ``self.group`` is
        ``(branches, pairing)``.  ``LinkPrecodedPlan`` sets ``self.pairs`` and ``self.n_sub``: ``self.group`` is ``(branches,
        subband)``, the entry point takes ``pmi int32 [rows, n_sub]`` behind ``llr``, and ``(counts, loss, llr, pmi)`` is returned.
        ``LinkSicPlan`` sets ``self.n_stats``: the entry point takes ``stats int32 [groups, n_stats]`` behind ``llr``, and ``(counts,
        loss, llr, stats)`` is returned."""
        lib = lib or _lib.load()
        batch, ideal, est, keys, sigma = self._checked(ideal, est, keys, sigma)
        pairs = self.pairs
        shape = (self.group[0], 2) if pairs else self.group
        if batch % math.prod(shape):
            raise ValueError(f"a batch of {batch} frames is not a multiple of "
                             f"{' * '.join(('branches', '2' if pairs else 'streams')[:len(shape)])} = {' * '.join(map(str, shape))}")
        groups = batch // math.prod(shape)
        rows = groups if pairs else groups * math.prod(self.group[1:])
        seq = (self.slots, self.delay)                          # LinkPrecodedPlan with delayed feedback: compact output rows
        if seq[0] > 1:
            if groups % seq[0]:
                raise ValueError(f"a batch of {batch} frames is not a multiple of slots * 2 * branches = {seq[0]} * 2 * {shape[0]}")
            rows = groups // seq[0] * (seq[0] - seq[1])
        rho = _in_place("rho", rho, torch.float32, self.device, batch)
        per_group = [_in_place(name, t, torch.float32, self.device, groups) for name, t in per_group]
        factors = self._checked_factors(factors)
        counts = torch.empty((rows, 2), dtype=torch.int32, device=self.device)                  # the kernel writes every element
        loss = torch.empty((rows, factors.numel()), dtype=torch.float32, device=self.device)
        llr = torch.empty((rows, *self.grid, self.cfg.bits_per_symbol), dtype=torch.float32, device=self.device) if want_llr else None
        pmi = () if self.n_sub is None else (torch.empty((rows, self.n_sub), dtype=torch.int32, device=self.device),)
        if self.n_stats is not None:                            # one row per GROUP: the order is an element's, not a stream's
            pmi = (torch.empty((groups, self.n_stats), dtype=torch.int32, device=self.device),)
        _lib.check(getattr(lib, entry)(C.byref(self.link), ideal.data_ptr(), est.data_ptr(), keys.data_ptr(), sigma.data_ptr(),
                                       rho.data_ptr(), *(t.data_ptr() for t in per_group), factors.data_ptr(), factors.numel(),
                                       *self.group, *(seq if seq[0] > 1 else ()), counts.data_ptr(), loss.data_ptr(), _ptr(llr), *(t.data_ptr() for t in pmi), batch,
                                       _lib.current_stream_ptr(self.device)), lib)
        return (counts, loss, llr, *pmi)

    def __call__(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor, lib=None) -> torch.Tensor:
        lib = lib or _lib.load()
        batch, ideal, est, keys, sigma = self._checked(ideal, est, keys, sigma)
        counts = torch.empty((batch, 2), dtype=torch.int32, device=self.device)             # the kernel writes every element
        _lib.check(lib.aft_link_errors_f32(C.byref(self.link), ideal.data_ptr(), est.data_ptr(), keys.data_ptr(), sigma.data_ptr(),
                                           counts.data_ptr(), batch, _lib.current_stream_ptr(self.device)), lib)
        return counts


class LinkSoftPlan(LinkPlan):
    """The soft half of ``LinkPlan``'s link.  ``plan(ideal, est, keys, sigma, scale, factors, want_llr=False)`` -> ``(loss float32
    [batch, K], llr float32 [batch, S, T, m] or None)`` on the plan's device: the loss of each frame at each of the K factors and, when
    asked for, the max-log LLR of every sent bit (0 at the pilots); one ``ctypes`` call, one launch (``aft_link_soft_f32``) on the
    current stream, no synchronisation.  ``scale`` (float32, ``batch`` values) and ``factors`` (float32, 1 .. 8 values) live where
    ``keys`` and ``sigma`` may: on the plan's device or in pinned host memory.  Everything else as ``LinkPlan``."""
    cpu_path = "linksim.link_llrs_host"

    def __call__(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor, scale: torch.Tensor,
                 factors: torch.Tensor, want_llr: bool = False, lib=None):
        lib = lib or _lib.load()
        batch, ideal, est, keys, sigma = self._checked(ideal, est, keys, sigma)
        scale = _in_place("scale", scale, torch.float32, self.device, batch)
        factors = self._checked_factors(factors)
        loss = torch.empty((batch, factors.numel()), dtype=torch.float32, device=self.device)   # the kernel writes every element
        llr = torch.empty((batch, *self.grid, self.cfg.bits_per_symbol), dtype=torch.float32, device=self.device) if want_llr else None
        _lib.check(lib.aft_link_soft_f32(C.byref(self.link), ideal.data_ptr(), est.data_ptr(), keys.data_ptr(), sigma.data_ptr(),
                                         scale.data_ptr(), factors.data_ptr(), factors.numel(), loss.data_ptr(), _ptr(llr), batch,
                                         _lib.current_stream_ptr(self.device)), lib)
        return loss, llr


class LinkMrcPlan(LinkPlan):
    """Receive diversity on ``LinkPlan``'s link: maximum-ratio combining over ``branches`` consecutive frames (``linksim``: "the
    diversity link").  ``plan(ideal, est, keys, sigma, rho, scale, factors, want_llr=False)`` -> ``(counts int32 [G, 2], loss float32
    [G, K], llr float32 [G, S, T, m] or None)`` for the ``G = batch / branches`` groups on the plan's device: three ``torch.empty``
    at the most, one ``ctypes`` call, one launch (``aft_link_mrc_f32``) on the current stream, no synchronisation.  ``rho`` (float32,
    ``batch`` values) and ``scale`` (float32, ``G`` values: the leaders') are ``linksim.branch_weights``'; they and ``factors`` live
    where ``keys`` and ``sigma`` may.  Everything else as ``LinkSoftPlan``."""
    cpu_path = "linksim.link_mrc_host"

    def __init__(self, cfg, device: torch.device, branches: int) -> None:
        super().__init__(cfg, device)
        if isinstance(branches, bool) or not isinstance(branches, int) or not 1 <= branches <= _abi.AFT_LINK_MAX_BRANCHES:
            raise ValueError(f"branches = {branches!r}: an integer in 1 .. {_abi.AFT_LINK_MAX_BRANCHES}")
        self.branches, self.group = branches, (branches,)

    def __call__(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor, rho: torch.Tensor,
                 scale: torch.Tensor, factors: torch.Tensor, want_llr: bool = False, lib=None):
        return self._grouped("aft_link_mrc_f32", ideal, est, keys, sigma, rho, [("scale", scale)], factors, want_llr, lib)


class LinkObservePlan(LinkMrcPlan):
    """The decision-directed observation on ``LinkMrcPlan``'s groups (``linksim.link_observe_host`` is the definition).
    ``plan(ideal, est, keys, sigma, rho, pilots)`` -> ``(z complex64 [batch, S, T], decisions uint8 [G, S, T], symbol_errors int32
    [G])`` on the plan's device: three ``torch.empty``, one ``ctypes`` call, one launch (``aft_link_observe_f32``) on the current
    stream, no synchronisation.  ``pilots`` complex64 ``[batch, Ps, Pt]`` live on the plan's device; ``source``: ``"decided"`` or
    ``"sent"``.  Everything else as ``LinkMrcPlan``."""
    cpu_path = "linksim.link_observe_host"

    def __init__(self, cfg, device: torch.device, branches: int = 1, source: str = "decided") -> None:
        from .linksim import _source
        super().__init__(cfg, device, branches)
        self.source = _source(source)
        self.pilot = tuple(cfg.sim.pilot)

    def __call__(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor, rho: torch.Tensor,
                 pilots: torch.Tensor, lib=None):
        lib = lib or _lib.load()
        batch, ideal, est, keys, sigma = self._checked(ideal, est, keys, sigma)
        if batch % self.branches:
            raise ValueError(f"a batch of {batch} frames is not a multiple of branches = {self.branches}")
        groups = batch // self.branches
        rho = _in_place("rho", rho, torch.float32, self.device, batch)
        if tuple(pilots.shape) != (batch, *self.pilot) or pilots.dtype != torch.complex64 or pilots.device != self.device:
            raise ValueError(f"pilots must be complex64 ({batch}, {self.pilot[0]}, {self.pilot[1]}) on {self.device}, got {pilots.dtype} "
                             f"{tuple(pilots.shape)} on {pilots.device}")
        pilots = pilots.contiguous()
        z = torch.empty((batch, *self.grid), dtype=torch.complex64, device=self.device)          # the kernel writes every element
        decisions = torch.empty((groups, *self.grid), dtype=torch.uint8, device=self.device)
        errors = torch.empty((groups,), dtype=torch.int32, device=self.device)
        _lib.check(lib.aft_link_observe_f32(C.byref(self.link), ideal.data_ptr(), est.data_ptr(), keys.data_ptr(), sigma.data_ptr(),
                                            rho.data_ptr(), pilots.data_ptr(), self.source, self.branches, z.data_ptr(),
                                            decisions.data_ptr(), errors.data_ptr(), batch, _lib.current_stream_ptr(self.device)), lib)
        return z, decisions, errors


class LinkSmPlan(LinkPlan):
    """Two-stream spatial multiplexing on ``LinkPlan``'s link: linear ZF / MMSE detection of ``streams = 2`` transmit streams on
    ``branches`` receive antennas (``linksim``: "the spatial-multiplexing link"); frame ``g N R + r N + s`` of a batch is the pair
    (antenna ``r``, stream ``s``) of group ``g``.  ``plan(ideal, est, keys, sigma, rho, scale, reg, factors, want_llr=False)`` ->
    ``(counts int32 [G N, 2], loss float32 [G N, K], llr float32 [G N, S, T, m] or None)`` for the ``G = batch / (branches streams)``
    groups on the plan's device, row ``g N + s`` stream ``s`` of group ``g`` (its key is frame ``(0, s)``'s): three ``torch.empty`` at
    the most, one ``ctypes`` call, one launch (``aft_link_sm_f32``) on the current stream, no synchronisation.  ``rho`` (float32,
    ``batch`` values), ``scale`` and ``reg`` (float32, ``G`` values: the leaders' LLR scale and the regulariser, 0 for zero forcing
    and ``1 / scale`` for MMSE) are ``linksim.sm_weights``'; they and ``factors`` live where ``keys`` and ``sigma`` may.  Everything
    else as ``LinkMrcPlan``."""
    cpu_path = "linksim.link_sm_host"

    def __init__(self, cfg, device: torch.device, branches: int, streams: int = 2) -> None:
        super().__init__(cfg, device)
        if isinstance(streams, bool) or not isinstance(streams, int) or streams != _abi.AFT_LINK_MAX_STREAMS:
            raise ValueError(f"streams = {streams!r}: the spatial-multiplexing link separates {_abi.AFT_LINK_MAX_STREAMS} streams")
        if isinstance(branches, bool) or not isinstance(branches, int) or not 2 <= branches <= _abi.AFT_LINK_MAX_BRANCHES:
            raise ValueError(f"branches = {branches!r}: an integer in 2 .. {_abi.AFT_LINK_MAX_BRANCHES} (one antenna cannot separate "
                             f"{streams} streams)")
        self.branches, self.streams, self.group = branches, streams, (branches, streams)

    def __call__(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor, rho: torch.Tensor,
                 scale: torch.Tensor, reg: torch.Tensor, factors: torch.Tensor, want_llr: bool = False, lib=None):
        return self._grouped("aft_link_sm_f32", ideal, est, keys, sigma, rho, [("scale", scale), ("reg", reg)], factors, want_llr, lib)


class LinkJointPlan(LinkSmPlan):
    """Joint max-log detection on ``LinkSmPlan``'s link and layout (``linksim``: "the joint link"): the exact max-log LLR of every bit
    of both streams.  ``plan(ideal, est, keys, sigma, rho, scale, factors, want_llr=False)`` -> ``LinkSmPlan``'s three tensors: three
    ``torch.empty`` at the most, one ``ctypes`` call, one launch (``aft_link_joint_f32``) on the current stream, no synchronisation.
    There is no regulariser; everything else as ``LinkSmPlan``."""
    cpu_path = "linksim.link_joint_host"

    def __call__(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor, rho: torch.Tensor,
                 scale: torch.Tensor, factors: torch.Tensor, want_llr: bool = False, lib=None):
        return self._grouped("aft_link_joint_f32", ideal, est, keys, sigma, rho, [("scale", scale)], factors, want_llr, lib)


class LinkSicPlan(LinkSmPlan):
    """Ordered successive cancellation on ``LinkSmPlan``'s link and layout (``linksim``: "the successive-cancellation link"): per
    element the stream with the larger Gram diagonal is detected by the linear detector, its decided symbol is cancelled from the
    matched sums, and the other stream is combined as a diversity link.  ``plan(ideal, est, keys, sigma, rho, scale, reg, factors,
    want_llr=False)`` -> ``LinkSmPlan``'s three tensors, indexed by stream, and ``stats int32 [G, 3]`` per group (data elements
    detected in swapped order, first decisions with a symbol error, of those the elements whose other stream is wrong too): four
    ``torch.empty`` at the most, one ``ctypes`` call, one launch (``aft_link_sic_f32``) on the current stream, no synchronisation.
    ``reg`` is any float32 ``>= 0`` per group (``linksim.detector_reg(scale, "mmse")`` for MMSE-SIC); everything else as
    ``LinkSmPlan``."""
    cpu_path = "linksim.link_sic_host"
    n_stats = 3

    def __call__(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor, rho: torch.Tensor,
                 scale: torch.Tensor, reg: torch.Tensor, factors: torch.Tensor, want_llr: bool = False, lib=None):
        return self._grouped("aft_link_sic_f32", ideal, est, keys, sigma, rho, [("scale", scale), ("reg", reg)], factors, want_llr, lib)


def _strided_words(name: str, t: torch.Tensor, device: torch.device, count: int) -> Tuple[int, int]:
    """``(address, stride in int32 units)`` of the int32 words a kernel on ``device`` reads IN PLACE through a one-dimensional view of
    ``count`` elements with a positive stride -- a column of the decoder's counts, say -- on the device or in pinned host memory."""
    if not torch.is_tensor(t) or t.dtype != torch.int32:
        raise ValueError(f"{name} must be torch.int32, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if t.dim() != 1 or t.numel() != count:
        raise ValueError(f"{name} must hold one value per row ({count}) in one dimension, got shape {tuple(t.shape)}")
    stride = t.stride(0) if count > 1 else 1
    if stride < 1:
        raise ValueError(f"{name} must be read at a stride of at least 1 (its view has stride {stride})")
    if not _readable_in_place(t, device):
        raise ValueError(f"{name} must live on {device} or in pinned host memory (it is on {t.device}, not pinned)")
    return t.data_ptr(), stride


class LinkCancelPlan(LinkSmPlan):
    """The second pass of codeword-level cancellation on ``LinkSmPlan``'s link and layout (``linksim``: "the codeword-cancellation
    link"): a stream whose first-pass decoding failed while the other stream's passed is detected again after the acknowledged
    stream's SENT symbol has left its matched sum.  ``plan(ideal, est, keys, sigma, rho, scale, failed, factors, want_llr=False,
    want_state=True)`` -> ``LinkSmPlan``'s three tensors -- zeros for every stream that is not detected again -- and ``state int32
    [G, 2]`` (1 where a stream was detected again; None without ``want_state``): four ``torch.empty`` at the most, one ``ctypes``
    call, one launch (``aft_link_cancel_f32``) on the current stream, no synchronisation.  ``failed`` is a one-dimensional int32 view
    of ``2 G`` first-pass block-error counts, row ``g 2 + s`` stream ``s`` of group ``g``, with any positive stride -- column 1 of
    ``LinkLdpcPlan``'s counts as it stands -- on the plan's device or in pinned host memory; the kernel reads it in place.  There is no
    ``reg``; everything else as ``LinkSmPlan``."""
    cpu_path = "linksim.link_cancel_host"

    def __call__(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor, rho: torch.Tensor,
                 scale: torch.Tensor, failed: torch.Tensor, factors: torch.Tensor, want_llr: bool = False, want_state: bool = True,
                 lib=None):
        lib = lib or _lib.load()
        batch, ideal, est, keys, sigma = self._checked(ideal, est, keys, sigma)
        width = self.branches * self.streams
        if batch % width:
            raise ValueError(f"a batch of {batch} frames is not a multiple of branches * streams = {self.branches} * {self.streams}")
        groups = batch // width
        rows = groups * self.streams
        rho = _in_place("rho", rho, torch.float32, self.device, batch)
        scale = _in_place("scale", scale, torch.float32, self.device, groups)
        failed_ptr, failed_stride = _strided_words("failed", failed, self.device, rows)
        factors = self._checked_factors(factors)
        counts = torch.empty((rows, 2), dtype=torch.int32, device=self.device)                  # the kernel writes every element
        loss = torch.empty((rows, factors.numel()), dtype=torch.float32, device=self.device)
        llr = torch.empty((rows, *self.grid, self.cfg.bits_per_symbol), dtype=torch.float32, device=self.device) if want_llr else None
        state = torch.empty((groups, self.streams), dtype=torch.int32, device=self.device) if want_state else None
        _lib.check(lib.aft_link_cancel_f32(C.byref(self.link), ideal.data_ptr(), est.data_ptr(), keys.data_ptr(), sigma.data_ptr(),
                                           rho.data_ptr(), scale.data_ptr(), factors.data_ptr(), factors.numel(), self.branches,
                                           self.streams, failed_ptr, failed_stride, counts.data_ptr(), loss.data_ptr(), _ptr(llr),
                                           _ptr(state), batch, _lib.current_stream_ptr(self.device)), lib)
        return counts, loss, llr, state


class LinkAlamoutiPlan(LinkPlan):
    """Transmit diversity on ``LinkPlan``'s link: two transmit antennas send ONE stream as Alamouti pairs over adjacent data symbols
    (``pairing="time"``) or subcarriers (``"frequency"``) and ``branches`` receive antennas combine (``linksim``: "the transmit-diversity
    link"); frame ``g 2R + r 2 + s`` of a batch is the pair (receive antenna ``r``, transmit antenna ``s``) of group ``g``.
    ``plan(ideal, est, keys, sigma, rho, scale, factors, want_llr=False)`` -> ``(counts int32 [G, 2], loss float32 [G, K], llr float32
    [G, S, T, m] or None)`` for the ``G = batch / (2 branches)`` groups on the plan's device: three ``torch.empty`` at the most, one
    ``ctypes`` call, one launch (``aft_link_alamouti_f32``) on the current stream, no synchronisation.  ``rho`` (float32, ``batch``
    values) and ``scale`` (float32, ``G`` values: the leaders') are ``linksim.alamouti_weights``'; they and ``factors`` live where
    ``keys`` and ``sigma`` may.  Everything else as ``LinkMrcPlan``."""
    cpu_path = "linksim.link_alamouti_host"
    pairs = True

    def __init__(self, cfg, device: torch.device, branches: int, pairing: str = "time") -> None:
        super().__init__(cfg, device)
        from .linksim import PAIRINGS
        if not isinstance(pairing, str) or pairing not in PAIRINGS:
            raise ValueError(f"pairing = {pairing!r}: one of {PAIRINGS}")
        if isinstance(branches, bool) or not isinstance(branches, int) or not 1 <= branches <= _abi.AFT_LINK_MAX_BRANCHES:
            raise ValueError(f"branches = {branches!r}: an integer in 1 .. {_abi.AFT_LINK_MAX_BRANCHES}")
        self.branches, self.pairing = branches, pairing
        self.group = (branches, (_abi.AFT_LINK_PAIR_TIME, _abi.AFT_LINK_PAIR_FREQUENCY)[PAIRINGS.index(pairing)])

    def __call__(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor, rho: torch.Tensor,
                 scale: torch.Tensor, factors: torch.Tensor, want_llr: bool = False, lib=None):
        return self._grouped("aft_link_alamouti_f32", ideal, est, keys, sigma, rho, [("scale", scale)], factors, want_llr, lib)


class LinkPrecodedPlan(LinkPlan):
    """Closed-loop rank-1 precoding on ``LinkPlan``'s link: two transmit antennas send ONE stream co-phased by a codebook precoder
    ``(1, q)``, ``q`` one of ``1, -1, j, -j``, which the receiver picks per subband of ``subband`` subcarriers from the estimates, and
    ``branches`` receive antennas combine (``linksim``: "the closed-loop link"); frame ``g 2R + r 2 + s`` of a batch is the pair
    (receive antenna ``r``, transmit antenna ``s``) of group ``g``.  ``plan(ideal, est, keys, sigma, rho, scale, factors,
    want_llr=False)`` -> ``(counts int32 [G, 2], loss float32 [G, K], llr float32 [G, S, T, m] or None, pmi int32 [G, n_sub])`` for the
    ``G = batch / (2 branches)`` groups on the plan's device, ``n_sub = ceil(S / subband)``: four ``torch.empty`` at the most, one
    ``ctypes`` call, one launch (``aft_link_precoded_f32``) on the current stream, no synchronisation.  ``rho`` (float32, ``batch``
    values) and ``scale`` (float32, ``G`` values: the leaders') are ``linksim.precoding_weights``'; they and ``factors`` live where
    ``keys`` and ``sigma`` may.  Everything else as ``LinkMrcPlan``.

    Delayed feedback: with ``slots = K > 1`` the batch is whole sequences of K groups (the slots of ``ChannelSimConfig(slots=K)``) and
    slot ``k >= delay`` is sent with the PMIs selected from slot ``k - delay`` of its sequence; slots ``k < delay`` are warm-up.  The four
    outputs have ``(G / K) (K - delay)`` rows, row ``seq (K - delay) + (k - delay)``, ``pmi`` the APPLIED indices; the inputs, ``scale``
    included, stay indexed by input frame or group.  One launch of ``aft_link_precoded_delayed_f32``; with ``slots = 1`` (then ``delay =
    0``) the launch is ``aft_link_precoded_f32`` as it was."""
    cpu_path = "linksim.link_precoded_host"
    pairs = True

    def __init__(self, cfg, device: torch.device, branches: int, subband: int, slots: int = 1, delay: int = 0) -> None:
        super().__init__(cfg, device)
        if any(isinstance(v, bool) or not isinstance(v, int) for v in (slots, delay)) or slots < 1 or not 0 <= delay < slots:
            raise ValueError(f"slots = {slots!r}, delay = {delay!r}: integers with slots >= 1 and 0 <= delay < slots")
        self.slots, self.delay = slots, delay
        if isinstance(branches, bool) or not isinstance(branches, int) or not 1 <= branches <= _abi.AFT_LINK_MAX_BRANCHES:
            raise ValueError(f"branches = {branches!r}: an integer in 1 .. {_abi.AFT_LINK_MAX_BRANCHES}")
        S = self.grid[0]
        if isinstance(subband, bool) or not isinstance(subband, int) or not 1 <= subband <= S:
            raise ValueError(f"subband = {subband!r}: an integer in 1 .. {S} subcarriers")
        self.n_sub = -(-S // subband)
        if self.n_sub > _abi.AFT_LINK_MAX_SUBBANDS:
            raise ValueError(f"subband = {subband} makes {self.n_sub} subbands of the {S} subcarriers, more than {_abi.AFT_LINK_MAX_SUBBANDS}")
        self.branches, self.subband, self.group = branches, subband, (branches, subband)

    def __call__(self, ideal: torch.Tensor, est: torch.Tensor, keys: torch.Tensor, sigma: torch.Tensor, rho: torch.Tensor,
                 scale: torch.Tensor, factors: torch.Tensor, want_llr: bool = False, lib=None):
        if self.slots == 1:
            return self._grouped("aft_link_precoded_f32", ideal, est, keys, sigma, rho, [("scale", scale)], factors, want_llr, lib)
        return self._grouped("aft_link_precoded_delayed_f32", ideal, est, keys, sigma, rho, [("scale", scale)], factors, want_llr, lib)


class _DecoderPlan:
    """What the decoder plans share: the code's link struct and LLR shape, and a call that checks ``llr`` and ``keys``, allocates
    ``counts int32 [groups, width]`` and, when asked for, ``bits uint8 [groups, B, K]`` (a group is one frame, or the HARQ link's
    ``rounds`` frames), and makes the one ``ctypes`` call.  A subclass
    names its config type, its CPU path, its entry point and the width of its counts, and gives the code's arguments as ``self.args``."""
    config = cpu_path = entry = None
    width = 2
    frames_per_group = 1                                        # the frames behind one row of counts (the HARQ link: its rounds)

    def __init__(self, code, device: torch.device) -> None:
        from . import linksim
        name = type(self).__name__
        if not isinstance(code, getattr(linksim, self.config)):
            raise ValueError(f"{name} needs a linksim.{self.config} (got {type(code).__name__})")
        self.device = _hip_device(device, name, self.cpu_path)
        self.code = code
        self.link = code.link.to_struct()                       # validated by the config itself; the entry point checks again
        self.shape = (*code.link.sim.ofdm, code.link.bits_per_symbol)

    def __call__(self, llr: torch.Tensor, keys: torch.Tensor, want_bits: bool = False, lib=None, *, _entry=None, _selection=None):
        """``_entry`` / ``_selection``: a subclass's second entry point and what it takes between the code's arguments and ``counts``
        (``LinkLdpcPlan``'s mask), as a function of the batch."""
        lib = lib or _lib.load()
        if llr.dim() != 4 or tuple(llr.shape[1:]) != self.shape or llr.shape[0] < 1:
            raise ValueError(f"Expected llr shape (B >= 1, {self.shape[0]}, {self.shape[1]}, {self.shape[2]}), got {tuple(llr.shape)}")
        if llr.dtype != torch.float32:
            raise ValueError(f"llr must be float32, got {llr.dtype}")
        if llr.device != self.device:
            raise ValueError(f"llr must live on {self.device} (it is on {llr.device})")
        batch = llr.shape[0]
        llr = llr.contiguous()                                  # held by the caller until after the launch is enqueued
        keys = _in_place("keys", keys, torch.int64, self.device, batch)
        if batch % self.frames_per_group:
            raise ValueError(f"a batch of {batch} frames is not a multiple of rounds = {self.frames_per_group}")
        groups = batch // self.frames_per_group
        selection = () if _selection is None else _selection(batch)
        counts = torch.empty((groups, self.width), dtype=torch.int32, device=self.device)   # the kernel writes every element
        bits = torch.empty((groups, self.code.blocks, self.code.info_bits), dtype=torch.uint8, device=self.device) if want_bits else None
        _lib.check(getattr(lib, _entry or self.entry)(C.byref(self.link), llr.data_ptr(), keys.data_ptr(), *self.args, *selection,
                                                      counts.data_ptr(), _ptr(bits), batch, _lib.current_stream_ptr(self.device)), lib)
        return counts, bits


class LinkDecodePlan(_DecoderPlan):
    """A coded link (``linksim.CodeConfig``) turned into ``aft_link_decode_f32``'s arguments ONCE.  ``plan(llr, keys, want_bits=False)``
    -> ``(counts int32 [batch, 2] = (information-bit errors, block errors) per frame, bits uint8 [batch, B, K] or None)`` on the plan's
    device: one ``ctypes`` call, one launch on the current stream, no synchronisation.  ``llr`` float32 ``[batch,S,T,m]`` (what
    ``LinkSoftPlan`` returns with ``want_llr``) lives on the plan's device; ``keys`` (int64, ``batch`` values) there or in pinned host
    memory, which the kernel reads in place.  The plan trusts its caller in one thing only: its device is the current one."""
    config, cpu_path, entry = "CodeConfig", "linksim.link_decode_host", "aft_link_decode_f32"

    def __init__(self, code, device: torch.device) -> None:
        super().__init__(code, device)
        self.args = (code.info_bits, code.rate_code, code.stride, code.stride_inverse, code.qgain)


class LinkLdpcPlan(_DecoderPlan):
    """An LDPC-coded link (``linksim.LdpcConfig``) turned into ``aft_link_ldpc_f32``'s arguments ONCE.  ``plan(llr, keys,
    want_bits=False)`` -> ``(counts int32 [batch, 3] = (information-bit errors, block errors, iterations summed over the blocks) per
    frame, bits uint8 [batch, B, K] or None)`` on the plan's device: one ``ctypes`` call, one launch on the current stream, no
    synchronisation.  Operands as ``LinkDecodePlan``'s.  The plan trusts its caller in one thing only: its device is the current one."""
    config, cpu_path, entry, width = "LdpcConfig", "linksim.link_ldpc_host", "aft_link_ldpc_f32", 3

    def __init__(self, code, device: torch.device) -> None:
        super().__init__(code, device)
        kb = code.base_cols - code.base_rows
        self.shifts = (C.c_int32 * (code.base_rows * kb))(*(v for row in code.shifts for v in row))      # host memory, read per call
        self.args = (code.base_rows, code.base_cols, C.addressof(self.shifts), code.stride, code.stride_inverse, code.qgain, code.offset,
                     code.max_iters)

    def __call__(self, llr: torch.Tensor, keys: torch.Tensor, want_bits: bool = False, lib=None, mask: Optional[torch.Tensor] = None):
        """``mask=None``: ``aft_link_ldpc_f32``.  ``mask``: a one-dimensional int32 view of ``batch`` words with any positive stride, on
        the plan's device or in pinned host memory, read in place by ``aft_link_ldpc_masked_f32`` -- the same kernel body --: a frame
        whose word is 0 is not decoded and gets counts ``(0, 0, 0)`` and zero bits; every other frame gets ``aft_link_ldpc_f32``'s
        outputs, bit for bit."""
        if mask is None:
            return super().__call__(llr, keys, want_bits, lib)
        return super().__call__(llr, keys, want_bits, lib, _entry="aft_link_ldpc_masked_f32",
                                _selection=lambda batch: _strided_words("mask", mask, self.device, batch))


class LinkHarqPlan(_DecoderPlan):
    """A HARQ link (``linksim.HarqConfig``) turned into ``aft_link_harq_f32``'s arguments ONCE.  ``plan(llr, keys, want_bits=False)`` ->
    ``(counts int32 [G, 7], bits uint8 [G, B, K] or None)`` for the ``G = batch / rounds`` groups on the plan's device (``linksim``:
    "The HARQ link" names the seven columns): one ``ctypes`` call, one launch on the current stream, no synchronisation.  ``llr``
    float32 ``[batch,S,T,m]`` and ``keys`` as ``LinkDecodePlan``'s, ``batch`` a multiple of ``rounds``; the shift and start tables are
    host arrays kept on the plan.  The plan trusts its caller in one thing only: its device is the current one."""
    config, cpu_path, entry, width = "HarqConfig", "linksim.link_harq_host", "aft_link_harq_f32", _abi.AFT_LINK_HARQ_COUNTS

    def __init__(self, harq, device: torch.device) -> None:
        super().__init__(harq, device)
        code = harq.code
        kb = code.base_cols - code.base_rows
        self.frames_per_group = harq.rounds
        self.shifts = (C.c_int32 * (code.base_rows * kb))(*(v for row in code.shifts for v in row))      # host memory, read per call
        self.starts = (C.c_int32 * harq.rounds)(*harq.starts)
        self.args = (code.base_rows, code.base_cols, C.addressof(self.shifts), harq.tx_cols, harq.rounds, C.addressof(self.starts),
                     harq.stride, harq.stride_inverse, code.qgain, code.offset, code.max_iters)


def ls_mse_db(ls: torch.Tensor, ideal: torch.Tensor) -> torch.Tensor:
    """Per-frame LS-baseline MSE in dB, float32 [B] (reference utils.py:248-261 per file)."""
    lib = _lib.load()
    if ls.dtype != torch.complex64 or ideal.dtype != torch.complex64 or ls.shape != ideal.shape or ls.dim() != 3:
        raise ValueError("ls / ideal must be complex64 [B, S, T] of equal shape")
    B, n = ls.shape[0], ls.shape[1] * ls.shape[2]
    db = torch.empty(B, dtype=torch.float32, device=ls.device)
    ls, ideal = ls.contiguous(), ideal.contiguous()      # held until after the launch is enqueued
    _lib.check(lib.aft_ls_mse_db_f32(torch.view_as_real(ls).data_ptr(),
                                     torch.view_as_real(ideal).data_ptr(), db.data_ptr(), B, n,
                                     _lib.current_stream_ptr(ls.device)))
    return db
