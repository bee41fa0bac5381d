"""A direct forward call of the training layer and its tape, for the tests that read the tape (helper module: no tests here)."""
import ctypes as C

import torch

from adafortitran_amd import _abi


def forward_tape(cfg, ps, x, p, seed):
    """aft_encoder_layer_fwd_train_f32 called directly: the layer output and the tape's regions (plan_tape's order, each rounded
    up to 64 floats)."""
    from adafortitran_amd import _lib
    from adafortitran_amd.training import _layer_struct
    lib = _lib.load()
    planes, tokens, d = x.shape
    heads, rows, batch = cfg.num_head, planes * tokens, planes // 2
    params = [q.cuda().contiguous() for q in ps]
    x = x.cuda().contiguous()
    out = torch.empty_like(x)
    tape = torch.zeros(lib.aft_encoder_tape_bytes(C.byref(cfg), batch), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(lib.aft_encoder_train_scratch_bytes(C.byref(cfg), batch), dtype=torch.uint8, device="cuda")
    w = _layer_struct(_abi.AftLayerWeights, params)
    _lib.check(lib.aft_encoder_layer_fwd_train_f32(C.byref(cfg), C.byref(w), x.data_ptr(), out.data_ptr(), tape.data_ptr(), tape.numel(),
                                                   scratch.data_ptr(), scratch.numel(), batch, p, seed, _lib.current_stream_ptr(x.device)))
    torch.cuda.synchronize()
    layout = (("qkv", 3 * d), ("attn", d), ("lse", heads), ("s1", d), ("st1", 2), ("x1", d), ("a", 2 * d), ("hd", 2 * d), ("s2", d),
              ("st2", 2))
    f, off, seg = tape.view(torch.float32), 0, {"out": out.cpu().numpy(), "x": x.cpu().numpy().reshape(rows, d)}
    for name, cols in layout:
        seg[name] = f[off:off + rows * cols].reshape(rows, cols).cpu().numpy()
        off += (rows * cols + 63) // 64 * 64
    return seg
