"""The steps the packed-rows calls of :class:`AudioCodec`, :class:`ProtectStream` and :class:`StreamingMDCT` share, each
written once: the refusals, the fixed-stride outputs, the one launch on packed input, and the tail of the compositions."""

from __future__ import annotations

import ctypes

import torch

from . import _host, _lib


def need_row_budget(codec, what):
    if codec.row_bits is None:
        raise ValueError("%s needs a codec with a row budget: make one with with_bitrate() or with_row_budget()" % what)


def check_pair(psy, data, index, of=""):
    """One ``(data, index)`` pair of packed rows: data uint8 [nbytes], index int64 [B, F, C] on data's device."""
    data = psy._check_quant_tensor(data, "data" + of, torch.uint8, ndim=1)
    return data, psy._check_quant_tensor(index, "index" + of, torch.int64, device=data.device, ndim=3)


def check_sources(psy, sources):
    """The ``(data, index)`` pairs of mix and route, every index of one shape on one device: (pairs, (B, F, C), device)."""
    pairs = []
    for i, (data, index) in enumerate(sources):
        data, index = check_pair(psy, data, index, " of source %d" % i)
        if pairs and (index.shape != pairs[0][1].shape or index.device != pairs[0][1].device):
            raise ValueError("index of source %d has shape %s on %s, that of source 0 shape %s on %s"
                             % (i, tuple(index.shape), index.device, tuple(pairs[0][1].shape), pairs[0][1].device))
        pairs.append((data, index))
    return pairs, tuple(pairs[0][1].shape), pairs[0][1].device


def packed_rows(data, index):
    """``ac_packed_rows`` of a checked pair."""
    return _lib.PackedRows(data.data_ptr(), data.numel(), index.data_ptr())


def source_rows(pairs):
    """The ``ac_packed_rows`` array of the checked pairs of :func:`check_sources`."""
    return (_lib.PackedRows * len(pairs))(*[packed_rows(d, ix) for d, ix in pairs])


def row_starts(shape, stride, dev):
    """index int64 ``shape`` = [B, F, C] of rows ``stride`` bytes apart: ``index[b, f, c] = ((b*F + f)*C + c) * stride``."""
    B, F, C = shape
    return (torch.arange(B * F * C, dtype=torch.int64, device=dev) * stride).view(B, F, C)


def outputs(shape, stride, dev, return_offset=False, lead=(), parts=1):
    """The results of a one-launch call into fixed-stride slots, uninitialised (the kernels write every byte): (data uint8
    ``lead`` + [B*F*C*stride], index, ``parts`` of fits bool ``lead`` + [B, F, C]), then ``parts`` of offset int16 with
    ``return_offset``.  For a shape without rows this is the whole result of the call."""
    B, F, C = shape
    index = row_starts(shape, stride, dev)
    data = torch.empty(lead + (B * F * C * stride,), dtype=torch.uint8, device=dev)
    out = (data, index) + tuple(torch.empty(lead + (B, F, C), dtype=torch.bool, device=dev) for _ in range(parts))
    if return_offset:
        out += tuple(torch.empty(lead + (B, F, C), dtype=torch.int16, device=dev) for _ in range(parts))
    return out


def fused_ex(codec, dev, src, flags, out0, out1, shape, stream=None):
    """``ac_encode_fused_ex`` on packed input: ``src`` a ctypes struct, ``out0`` a struct or a tensor, ``out1`` a struct, a
    tensor or None, ``shape`` the rows' [B, F, C]; enqueued on ``stream`` (a ``torch.cuda.Stream``) or the current stream."""
    # the structs are passed as objects, not addresses: this frame holds them (and what they point to) until the call is back
    B, F, C = shape
    p0 = out0.data_ptr() if isinstance(out0, torch.Tensor) else ctypes.addressof(out0)
    p1 = None if out1 is None else out1.data_ptr() if isinstance(out1, torch.Tensor) else ctypes.addressof(out1)
    with _host.on_device(dev):
        _lib.check(codec._lib.ac_encode_fused_ex(
            codec.mdct._plan(dev), codec.psy._plan(dev), ctypes.addressof(src), None, None, None, 0.0, flags, p0, p1, 0,
            B, F - 1, C, _host.stream_ptr(dev) if stream is None else ctypes.c_void_p(stream.cuda_stream)))


def repack(codec, src, flags, out, stride):
    """:func:`fused_ex` from ``src`` (under ``AC_IN_PACKED`` and ``flags``) into the slots, flags and offsets of
    :func:`outputs`' ``out``."""
    dst = _lib.PackedOut(out[0].data_ptr(), stride, out[2].data_ptr())
    fused_ex(codec, out[0].device, src, _lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED | flags, dst, out[3] if len(out) > 3 else None,
             tuple(out[1].shape))
    return out


def pack_quantized(psy, quantized, row_bytes, return_offset):
    """The tail of the compositions of transrate and mix: ``quantized`` = (codes, sf, offset, bits) at the budget -> the
    call's result at fixed row starts."""
    codes, sf, offset, bits = quantized
    B, _, _, C = codes.shape
    index = row_starts((B, codes.shape[1], C), row_bytes, codes.device)
    data, fits = pack_rows_of_codes(psy, codes, sf, bits, index, row_bytes)
    return (data, index, fits, offset) if return_offset else (data, index, fits)


def pack_rows_of_spectra(psy, X, thr, index, row_bytes):
    """The tail of the composition of packed rows, shared by :meth:`AudioCodec.encode_packed_rows` and
    :meth:`StreamingMDCT.encode_packed_rows_chunk`: ``psy.quantize_to_budget`` at the model's budget on X, thr [B, F, N, C] (on
    plain allocations: nothing here may wait for the device), rows longer than their slot marked, then the packer at the fixed
    row starts ``index`` into zero-filled data.  Returns (data uint8 [B*F*C*row_bytes], fits bool [B, F, C]); everything is
    enqueued on the current stream."""
    row_bits, min_offset = psy.row_budget
    codes, sf, _, bits = psy.quantize_to_budget(X, thr, row_bits, min_offset)
    return pack_rows_of_codes(psy, codes, sf, bits, index, row_bytes)


def pack_rows_of_codes(psy, codes, sf, bits, index, row_bytes):
    """The tail of :func:`pack_rows_of_spectra`, which the compositions of :meth:`AudioCodec.transrate_packed_rows` and
    :meth:`AudioCodec.mix_packed_rows` share: codes [B, F, N, C], sf (changed in place) and their packed lengths ``bits``
    [B, F, C] -> (data, fits)."""
    B, F, _, C = codes.shape
    dev = codes.device
    fits = bits <= 8 * row_bytes
    sf.masked_fill_(~fits.unsqueeze(2), -128)   # width 31 follows whatever the codes are
    data = torch.zeros((B * F * C * row_bytes,), dtype=torch.uint8, device=dev)
    with _host.on_device(dev):
        _lib.check(_lib.load().ac_pack(psy._plan(dev), _host.ptr(codes), _host.ptr(sf), _host.ptr(index), _host.ptr(data), B, F, C,
                                       _host.stream_ptr(dev)))
    return data, fits


def protect(codec, data, index, red_bits, return_offset, carry=None, stream=None):
    """:meth:`AudioCodec.protect_packed_rows` on a checked pair; with ``carry`` = (the half frame 0 takes its copy from, or
    None: the values of f = 0; the half that takes the copy of the last row) the chunk of
    :meth:`ProtectStream.protect_chunk`, enqueued on ``stream``.  Without rows nothing is enqueued and no half written."""
    B, F, C = shape = tuple(index.shape)
    dev, rb = data.device, codec.row_bytes
    sb = codec.protected_slot_bytes(red_bits)
    query = codec._lib.ac_protect_launches if carry is None else codec._lib.ac_protect_chunk_launches
    if index.numel() == 0 or query(codec.psy._plan(dev), C, red_bits) == 1:
        out = outputs(shape, sb, dev, return_offset, parts=2)
        if index.numel() == 0:
            return out
        dst = _lib.ProtectedOut(out[0].data_ptr(), rb, out[2].data_ptr(), red_bits, out[3].data_ptr(),
                                out[4].data_ptr() if return_offset else None, out[5].data_ptr() if return_offset else None)
        flags, halves = _lib.AC_IN_PACKED | _lib.AC_EMIT_PACKED | _lib.AC_EMIT_REDUNDANT, None
        if carry is not None:
            flags |= _lib.AC_EMIT_CARRY
            halves = _lib.ProtectCarry(*((None, None, None) if carry[0] is None else [t.data_ptr() for t in carry[0]]),
                                       *[t.data_ptr() for t in carry[1]])
        fused_ex(codec, dev, packed_rows(data, index), flags, dst, halves, shape, stream)
        return out
    # the composition: the rows transrated at both budgets, then copied into the two parts of every slot
    prim = codec.transrate_packed_rows(data, index, True)
    red = codec._redundant_codec(red_bits).transrate_packed_rows(data, index, True)
    red_rows = red[0].view(B, F, C, sb - rb)
    slots = torch.zeros((B, F, C, sb), dtype=torch.uint8, device=dev)
    slots[..., :rb] = prim[0].view(B, F, C, rb)
    slots[:, 1:, :, rb:] = red_rows[:, :-1]
    red_fits = torch.ones((B, F, C), dtype=torch.bool, device=dev)
    red_fits[:, 1:] = red[2][:, :-1]
    red_offset = None
    if return_offset or carry is not None:
        red_offset = torch.zeros((B, F, C), dtype=torch.int16, device=dev)
        red_offset[:, 1:] = red[3][:, :-1]
    if carry is not None:   # frame 0 from the carried half, the copy of the last row into the other half
        if carry[0] is not None:
            slots[:, 0, :, rb:], red_fits[:, 0], red_offset[:, 0] = carry[0]
        for kept, new in zip(carry[1], (red_rows, red[2], red[3])):
            kept.copy_(new[:, -1])
    out = (slots.view(-1), row_starts(shape, sb, dev), prim[2], red_fits)
    return out + (prim[3], red_offset) if return_offset else out
