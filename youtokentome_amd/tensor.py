"""Device tensors in, device tensors out: `BPE.encode_tensor` / `BPE.encode_text_tensor` / `BPE.text_lines_tensor` / `BPE.decode_tensor` /
`BPE.encode_subword_tensor` / `BPE.encode_text_subword_tensor` / `BPE.encode_spans_tensor` / `BPE.encode_text_spans_tensor` / `BPE.decode_text_tensor` / `BPE.parse_ids_tensor` / `BPE.id_counts_tensor` / `BPE.*blocks*_tensor` / `BPE.*batches*_tensor` on top
of the raw device layer of `bpe._Core` (include/yttm_mi355x.h: yttm_encode_device, yttm_encode_text_device, yttm_lines_*, yttm_encode_copy_*,
yttm_decode_device*, yttm_decode_copy_device).  torch is imported at call
time; the rest of the package does not need it.

The library works on a non-blocking stream of its own and returns after that stream has synchronised.  So the hand-over is: synchronise
torch's current stream (whatever produced the input tensors is done), call the library, and let it fill output tensors that torch
allocated -- torch owns all memory it sees."""
import collections

import numpy as np

from .bpe import _check_dropout


def _torch():
    import torch
    return torch


def _device_of(bpe, device):
    torch = _torch()
    own = torch.device("cuda", bpe.bpe_cython.device)
    if device is not None:
        want = torch.device(device)
        if want.type != "cuda" or (want.index is not None and want.index != own.index):
            raise ValueError("device %s is not the encoder's (%s)" % (want, own))
    return own


def _pad_id(bpe, padded, pad_id):
    """the value behind a row's last id: the caller's, else the model's <PAD>"""
    if padded and pad_id is None:
        pad_id = bpe.subword_to_id("<PAD>")
        if pad_id == -1 or bpe.id_to_subword(pad_id) != "<PAD>":
            raise ValueError("the model was trained without <PAD> (pad_id=-1): pass pad_id")
    return pad_id


def _synced(torch, dev, call, *args):
    """call(*args) once torch's current stream is done: the tensors the library is about to read are complete, those it fills are allocated"""
    torch.cuda.current_stream(dev).synchronize()
    return call(*args)


def _check_on(t, dev, what):
    if t.device.type != dev.type or t.device.index != dev.index:
        raise ValueError("%s is on %s, the encoder on %s" % (what, t.device, dev))


def _offsets_u64(torch, offsets, dev, what="offsets"):
    """int64 / uint64 offsets tensor -> contiguous tensor whose memory the library reads as uint64 (the values are below 2^63)"""
    if getattr(torch, "uint64", None) is not None and offsets.dtype == torch.uint64:
        offsets = offsets.view(torch.int64)
    if offsets.dtype != torch.int64:
        raise ValueError("%s must be an int64 or uint64 tensor" % what)
    _check_on(offsets, dev, what)
    return offsets.contiguous()


def _sentences_on(torch, sentences, dev):
    """list[str], or a pair (uint8 bytes [B], int64 / uint64 offsets [n + 1]) on the device -> (bytes, offsets, n, total bytes, longest sentence)"""
    if isinstance(sentences, (list, tuple)) and not (len(sentences) == 2 and hasattr(sentences[0], "data_ptr")):
        from .bpe import _pack
        blob, offs = _pack(list(sentences))
        n = len(offs) - 1
        lens = np.diff(offs.astype(np.int64)) if n else np.zeros(0, np.int64)
        total, longest_in = int(offs[-1]), int(lens.max()) if n else 0
        d_bytes = torch.frombuffer(bytearray(blob) if blob else bytearray(1), dtype=torch.uint8).to(dev)
        d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
    else:
        d_bytes, d_off = sentences
        if d_bytes.dtype != torch.uint8 or d_bytes.dim() != 1 or d_off.dim() != 1 or d_off.numel() < 1:
            raise ValueError("device input is a pair (uint8 bytes [B], int64 or uint64 offsets [n + 1])")
        _check_on(d_bytes, dev, "bytes")
        d_bytes, d_off = d_bytes.contiguous(), _offsets_u64(torch, d_off, dev)
        n = d_off.numel() - 1
        if n:
            total = int(d_off[-1])
            longest_in = int((d_off[1:] - d_off[:-1]).max())
            if int(d_off[0]) != 0:
                raise ValueError("offsets[0] must be 0")
        else:
            total = longest_in = 0
    return d_bytes, d_off, n, total, longest_in


def encode_tensor(bpe, sentences, bos=False, eos=False, reverse=False, dropout_prob=0, padded=True, width=None, pad_id=None, device=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, device)
    _check_dropout(dropout_prob)
    pad_id = _pad_id(bpe, padded, pad_id)
    d_bytes, d_off, n, total, longest_in = _sentences_on(torch, sentences, dev)
    n_ids, _ = _synced(torch, dev, core.encode_device_raw, d_bytes.data_ptr(), d_off.data_ptr(), n, total, longest_in, bos, eos, reverse, dropout_prob)
    return _take_encoded(torch, core, dev, n, n_ids, padded, width, pad_id)


def _take_encoded(torch, core, dev, n, n_ids, padded, width, pad_id):
    """the pending encode result of n sentences as tensors that torch owns"""
    core.pending_n_sent = n  # (id_counts_tensor counts this result)
    if not padded:
        ids = torch.empty(n_ids, dtype=torch.int32, device=dev)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        _synced(torch, dev, core.copy_encode_device, ids.data_ptr(), out_off.data_ptr(), n)
        return ids, out_off
    longest = core.encode_longest(n) if n else 0
    if width is None:
        width = longest
    elif width < longest:
        raise ValueError("width = %d is smaller than the longest row (%d ids)" % (width, longest))
    matrix = torch.empty((n, width), dtype=torch.int32, device=dev)
    lengths = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        _synced(torch, dev, core.copy_encode_padded, matrix.data_ptr(), lengths.data_ptr(), n, width, pad_id)
    return matrix, lengths


def _text_on(torch, text, dev):
    """1-D uint8 tensor on the encoder's device, or bytes-like (uploaded) -> (contiguous tensor, n_bytes)"""
    if isinstance(text, (bytes, bytearray, memoryview)):
        raw = bytearray(text)
        n = len(raw)
        return torch.frombuffer(raw if n else bytearray(1), dtype=torch.uint8).to(dev), n
    if not hasattr(text, "data_ptr") or text.dtype != torch.uint8 or text.dim() != 1:
        raise ValueError("text is a 1-D uint8 tensor on the encoder's device, or bytes / bytearray / memoryview")
    _check_on(text, dev, "text")
    return text.contiguous(), text.numel()


def encode_text_tensor(bpe, text, bos=False, eos=False, reverse=False, dropout_prob=0, padded=True, width=None, pad_id=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    _check_dropout(dropout_prob)
    pad_id = _pad_id(bpe, padded, pad_id)
    d_text, n_bytes = _text_on(torch, text, dev)
    n, n_ids, _ = _synced(torch, dev, core.encode_text_device_raw, d_text.data_ptr(), n_bytes, bos, eos, reverse, dropout_prob)
    return _take_encoded(torch, core, dev, n, n_ids, padded, width, pad_id)


def text_lines_tensor(bpe, text):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    d_text, n_bytes = _text_on(torch, text, dev)
    n, _, _ = _synced(torch, dev, core.lines_device_raw, d_text.data_ptr(), n_bytes)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    _synced(torch, dev, core.copy_lines_device, off.data_ptr(), n)
    return off


def decode_tensor(bpe, ids, lengths=None, offsets=None, ignore_ids=None, as_str=True):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    _check_on(ids, dev, "ids")
    if ids.dtype == torch.int64:
        ids = ids.to(torch.int32)
    elif ids.dtype != torch.int32:
        raise ValueError("ids must be an int32 or int64 tensor")
    if ids.dim() == 2:
        if offsets is not None:
            raise ValueError("offsets go with 1-D ids; a 2-D matrix takes lengths")
        n, width = ids.shape
        if n and width and ids.stride(1) != 1:
            ids = ids.contiguous()
        stride = ids.stride(0) if n > 1 and width else width  # (rows of a sliced matrix keep their distance: no copy)
        if stride < width:
            ids, stride = ids.contiguous(), width
        d_len = 0
        if lengths is not None:
            _check_on(lengths, dev, "lengths")
            if lengths.dim() != 1 or lengths.numel() != n:
                raise ValueError("lengths must have one entry per row")
            lengths = lengths.to(torch.int32).contiguous()
            d_len = lengths.data_ptr()
        n_bytes, _ = _synced(torch, dev, core.decode_device_padded_raw, ids.data_ptr(), n, width, stride, d_len or None, ignore_ids)
    elif ids.dim() == 1:
        if offsets is None or lengths is not None:
            raise ValueError("1-D ids take offsets [n + 1] (and no lengths)")
        offsets = _offsets_u64(torch, offsets, dev)
        ids = ids.contiguous()
        n = offsets.numel() - 1
        if n < 0:
            raise ValueError("offsets must have at least one entry")
        if n and (int(offsets[-1]) > ids.numel() or int(offsets[0]) < 0 or bool((offsets[1:] < offsets[:-1]).any())):
            raise ValueError("offsets must be non-decreasing and end inside ids")
        n_bytes, _ = _synced(torch, dev, core.decode_device_raw, ids.data_ptr(), offsets.data_ptr(), n, ids.numel(), ignore_ids)
    else:
        raise ValueError("ids must be 1-D (with offsets) or 2-D (padded)")
    return _take_text(torch, core, dev, n, n_bytes, as_str, errors="strict")


def _take_text(torch, core, dev, n, n_bytes, as_str, errors="replace"):
    """the pending text of n lines: list[str], or (uint8 text, int64 line_off [n + 1]) tensors that torch owns.  errors: a formatter's text may cut
    a sentence's invalid UTF-8 as it stood ("replace"); a decode's is the vocabulary's own ("strict")"""
    if as_str:
        raw, off = core.fetch_decode(n, n_bytes)
        raw, o = raw.tobytes(), off.tolist()
        return [raw[o[i]:o[i + 1]].decode(errors=errors) for i in range(n)]
    text = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    _synced(torch, dev, core.copy_decode_device, text.data_ptr(), out_off.data_ptr(), n)
    return text, out_off


def encode_subword_tensor(bpe, sentences, bos=False, eos=False, reverse=False, dropout_prob=0, device=None, as_str=False):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, device)
    _check_dropout(dropout_prob)
    d_bytes, d_off, n, total, longest_in = _sentences_on(torch, sentences, dev)
    _, n_text, _ = _synced(torch, dev, core.subword_device_raw, d_bytes.data_ptr(), d_off.data_ptr(), n, total, longest_in, bos, eos, reverse, dropout_prob)
    core.pending_n_sent = n
    return _take_text(torch, core, dev, n, n_text, as_str)


def encode_text_subword_tensor(bpe, text, bos=False, eos=False, reverse=False, dropout_prob=0, as_str=False):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    _check_dropout(dropout_prob)
    d_text, n_bytes = _text_on(torch, text, dev)
    n, _, n_text, _ = _synced(torch, dev, core.subword_text_device_raw, d_text.data_ptr(), n_bytes, bos, eos, reverse, dropout_prob)
    core.pending_n_sent = n
    return _take_text(torch, core, dev, n, n_text, as_str)


def _take_spans(torch, core, dev, n, n_ids, padded, width, pad_id):
    """the pending encode result of n sentences and its spans as tensors that torch owns"""
    first, second = _take_encoded(torch, core, dev, n, n_ids, padded, width, pad_id)
    if not padded:
        spans = torch.empty((n_ids, 2), dtype=torch.int32, device=dev)
        _synced(torch, dev, core.copy_spans_device, spans.data_ptr(), n)
        return first, second, spans
    spans = torch.empty((n, first.shape[1], 2), dtype=torch.int32, device=dev)
    if n:
        _synced(torch, dev, core.copy_spans_padded, spans.data_ptr(), n, first.shape[1])
    return first, second, spans


def encode_spans_tensor(bpe, sentences, bos=False, eos=False, reverse=False, dropout_prob=0, padded=True, width=None, pad_id=None, device=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, device)
    _check_dropout(dropout_prob)
    pad_id = _pad_id(bpe, padded, pad_id)
    d_bytes, d_off, n, total, longest_in = _sentences_on(torch, sentences, dev)
    n_ids, _ = _synced(torch, dev, core.spans_device_raw, d_bytes.data_ptr(), d_off.data_ptr(), n, total, longest_in, bos, eos, reverse, dropout_prob)
    return _take_spans(torch, core, dev, n, n_ids, padded, width, pad_id)


def encode_text_spans_tensor(bpe, text, bos=False, eos=False, reverse=False, dropout_prob=0, padded=True, width=None, pad_id=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    _check_dropout(dropout_prob)
    pad_id = _pad_id(bpe, padded, pad_id)
    d_text, n_bytes = _text_on(torch, text, dev)
    n, n_ids, _ = _synced(torch, dev, core.spans_text_device_raw, d_text.data_ptr(), n_bytes, bos, eos, reverse, dropout_prob)
    return _take_spans(torch, core, dev, n, n_ids, padded, width, pad_id)


def parse_ids_tensor(bpe, text, padded=False, width=None, pad_id=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    pad_id = _pad_id(bpe, padded, pad_id)
    d_text, n_bytes = _text_on(torch, text, dev)
    n, n_ids, _ = _synced(torch, dev, core.ids_parse_device_raw, d_text.data_ptr(), n_bytes)
    return _take_encoded(torch, core, dev, n, n_ids, padded, width, pad_id)


def decode_text_tensor(bpe, text, ignore_ids=None, as_str=True):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    d_text, n_bytes = _text_on(torch, text, dev)
    n, _, n_text, _ = _synced(torch, dev, core.decode_text_device_raw, d_text.data_ptr(), n_bytes, ignore_ids)
    core.pending_n_sent = n
    if as_str:
        return [s[:-1] for s in _take_text(torch, core, dev, n, n_text, True)]
    return _take_text(torch, core, dev, n, n_text, False)


def _ragged_ids(torch, dev, ids, lengths, offsets, padded):
    """ids as a 2-D matrix (with lengths) or 1-D with offsets -> (int32 ids back to back, offsets [n + 1], n, padded: the form the result takes)"""
    _check_on(ids, dev, "ids")
    if ids.dtype == torch.int64:
        ids = ids.to(torch.int32)
    elif ids.dtype != torch.int32:
        raise ValueError("ids must be an int32 or int64 tensor")
    if ids.dim() == 2:
        if offsets is not None:
            raise ValueError("offsets go with 1-D ids; a 2-D matrix takes lengths")
        n, w = ids.shape
        if lengths is None:
            lens = torch.full((n,), w, dtype=torch.int64, device=dev)
        else:
            _check_on(lengths, dev, "lengths")
            if lengths.dim() != 1 or lengths.numel() != n:
                raise ValueError("lengths must have one entry per row")
            lens = lengths.to(torch.int64).clamp(0, w)
        # the rows' ids back to back (the library's pass takes the ragged form)
        keep = torch.arange(w, device=dev).unsqueeze(0) < lens.unsqueeze(1)
        flat = ids[keep].contiguous()
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
        ids = flat
        if padded is None:
            padded = True
    elif ids.dim() == 1:
        if offsets is None or lengths is not None:
            raise ValueError("1-D ids take offsets [n + 1] (and no lengths)")
        offsets = _offsets_u64(torch, offsets, dev)
        ids = ids.contiguous()
        n = offsets.numel() - 1
        if n < 0:
            raise ValueError("offsets must have at least one entry")
        if n and (int(offsets[-1]) > ids.numel() or int(offsets[0]) != 0 or bool((offsets[1:] < offsets[:-1]).any())):
            raise ValueError("offsets must start at 0, be non-decreasing and end inside ids")
        if padded is None:
            padded = False
    else:
        raise ValueError("ids must be 1-D (with offsets) or 2-D (padded)")
    return ids, offsets, n, padded


def restrict_tensor(bpe, ids, lengths=None, offsets=None, reverse=False, padded=None, width=None, pad_id=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    ids, offsets, n, padded = _ragged_ids(torch, dev, ids, lengths, offsets, padded)
    pad_id = _pad_id(bpe, padded, pad_id)
    n_in = int(offsets[-1]) if n else 0
    n_out, _ = _synced(torch, dev, core.restrict_ids_device_raw, ids.data_ptr(), offsets.data_ptr(), n, n_in, reverse)
    return _take_encoded(torch, core, dev, n, n_out, padded, width, pad_id)


def byte_fallback_tensor(bpe, ids, text, lengths=None, offsets=None, reverse=False, padded=None, width=None, pad_id=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    ids, offsets, n, padded = _ragged_ids(torch, dev, ids, lengths, offsets, padded)
    d_bytes, d_soff, n_text, total, _ = _sentences_on(torch, text, dev)
    if n_text != n:
        raise ValueError("text holds %d sentences, ids %d" % (n_text, n))
    pad_id = _pad_id(bpe, padded, pad_id)
    n_in = int(offsets[-1]) if n else 0
    n_out, _ = _synced(torch, dev, core.byte_fallback_ids_device_raw, ids.data_ptr(), offsets.data_ptr(), d_bytes.data_ptr(), d_soff.data_ptr(), n, n_in,
                       total, reverse)
    return _take_encoded(torch, core, dev, n, n_out, padded, width, pad_id)


def split_added_tensor(bpe, text, offsets=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    d_bytes, d_off, n, total, _ = _sentences_on(torch, text if offsets is None else (text, offsets), dev)
    n_sub, _, _ = _synced(torch, dev, core.added_split_device_raw, d_bytes.data_ptr(), d_off.data_ptr(), n, total)
    first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    sub_off = torch.zeros(n_sub + 1, dtype=torch.int64, device=dev)
    tok = torch.empty(n_sub, dtype=torch.int32, device=dev)
    _synced(torch, dev, core.copy_added_split, first.data_ptr(), sub_off.data_ptr(), tok.data_ptr(), n, n_sub)
    return first, sub_off, tok


def id_counts_tensor(bpe, ids=None, n_bins=None, accumulate=False):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    n_bins = int(n_bins) if n_bins is not None else core.id_bound()
    if n_bins < 1:
        raise ValueError("n_bins must be positive")
    if ids is None:
        n = getattr(core, "pending_n_sent", None)
        if n is None:
            raise ValueError("id_counts_tensor: no *_tensor encode or parse call has left a result to count")
        _synced(torch, dev, core.id_counts_device_raw, n, n_bins, accumulate)
    else:
        if not hasattr(ids, "data_ptr") or ids.dtype != torch.int32:
            raise ValueError("ids must be an int32 tensor")
        _check_on(ids, dev, "ids")
        if not ids.is_contiguous():
            raise ValueError("ids must be contiguous")
        _synced(torch, dev, core.id_counts_ids_device_raw, ids.data_ptr(), ids.numel(), n_bins, accumulate)
    counts = torch.empty(n_bins + 1, dtype=torch.int64, device=dev)
    _synced(torch, dev, core.copy_id_counts_device, counts.data_ptr(), n_bins)
    return counts


# ---- training blocks (include/yttm_mi355x.h "Training blocks") ---------------------------------------------------------------------------------
Blocks = collections.namedtuple("Blocks", "rows seg pos frags row_frags")


def _blocks_args(bpe, seq_len, mode, pad_id, tail):
    core = bpe.bpe_cython
    if mode not in core.MODES:
        raise ValueError('mode must be "stream" or "whole"')
    if tail not in core.TAILS:
        raise ValueError('tail must be "pad", "keep" or "drop"')
    if int(seq_len) < 1:
        raise ValueError("seq_len must be positive")
    pad_id = _pad_id(bpe, tail == "pad", pad_id)
    return int(seq_len), core.MODES[mode], 0 if pad_id is None else int(pad_id), core.TAILS[tail]


def _take_blocks(torch, core, dev, n_rows, n_frags, seq_len):
    """the blocks slot as tensors that torch owns"""
    rows, seg, pos = (torch.empty((n_rows, seq_len), dtype=torch.int32, device=dev) for _ in range(3))
    frags = torch.empty((n_frags, 2), dtype=torch.int32, device=dev)
    row_frags = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    _synced(torch, dev, core.copy_blocks_device, rows.data_ptr(), seg.data_ptr(), pos.data_ptr(), frags.data_ptr(), row_frags.data_ptr(), n_rows, n_frags)
    return Blocks(rows, seg, pos, frags, row_frags)


def encode_blocks_tensor(bpe, sentences, seq_len, mode="stream", bos=False, eos=False, reverse=False, dropout_prob=0, pad_id=None, tail="pad", device=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, device)
    _check_dropout(dropout_prob)
    L, m, pad, t = _blocks_args(bpe, seq_len, mode, pad_id, tail)
    d_bytes, d_off, n, total, longest_in = _sentences_on(torch, sentences, dev)
    _synced(torch, dev, core.encode_device_raw, d_bytes.data_ptr(), d_off.data_ptr(), n, total, longest_in, bos, eos, reverse, dropout_prob)
    core.pending_n_sent = n
    n_rows, n_frags, _ = core.blocks_device_raw(n, L, m, pad, t)
    return _take_blocks(torch, core, dev, n_rows, n_frags, L)


def encode_text_blocks_tensor(bpe, text, seq_len, mode="stream", bos=False, eos=False, reverse=False, dropout_prob=0, pad_id=None, tail="pad"):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    _check_dropout(dropout_prob)
    L, m, pad, t = _blocks_args(bpe, seq_len, mode, pad_id, tail)
    d_text, n_bytes = _text_on(torch, text, dev)
    n, _, _ = _synced(torch, dev, core.encode_text_device_raw, d_text.data_ptr(), n_bytes, bos, eos, reverse, dropout_prob)
    core.pending_n_sent = n
    n_rows, n_frags, _ = core.blocks_device_raw(n, L, m, pad, t)
    return _take_blocks(torch, core, dev, n_rows, n_frags, L)


def blocks_tensor(bpe, ids=None, lengths=None, offsets=None, seq_len=0, mode="stream", pad_id=None, tail="pad"):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    L, m, pad, t = _blocks_args(bpe, seq_len, mode, pad_id, tail)
    if ids is None:
        n = getattr(core, "pending_n_sent", None)
        if n is None:
            raise ValueError("blocks_tensor: no *_tensor encode or parse call has left a result to pack")
        n_rows, n_frags, _ = _synced(torch, dev, core.blocks_device_raw, n, L, m, pad, t)
        return _take_blocks(torch, core, dev, n_rows, n_frags, L)
    if not hasattr(ids, "data_ptr") or ids.dtype != torch.int32:
        raise ValueError("ids must be an int32 tensor")
    _check_on(ids, dev, "ids")
    if ids.dim() == 2:
        if offsets is not None:
            raise ValueError("offsets go with 1-D ids; a 2-D matrix takes lengths")
        n, w = ids.shape
        if lengths is None:
            lens = torch.full((n,), w, dtype=torch.int64, device=dev)
        else:
            _check_on(lengths, dev, "lengths")
            if lengths.dim() != 1 or lengths.numel() != n:
                raise ValueError("lengths must have one entry per row")
            lens = lengths.to(torch.int64).clamp(0, w)
        keep = torch.arange(w, device=dev).unsqueeze(0) < lens.unsqueeze(1)  # the rows' ids back to back (the library's pass takes the ragged form)
        ids = ids[keep].contiguous()
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
    elif ids.dim() == 1:
        if offsets is None or lengths is not None:
            raise ValueError("1-D ids take offsets [n + 1] (and no lengths)")
        offsets = _offsets_u64(torch, offsets, dev)
        ids = ids.contiguous()
        n = offsets.numel() - 1
        if n < 0:
            raise ValueError("offsets must have at least one entry")
        if n and (int(offsets[-1]) > ids.numel() or int(offsets[0]) != 0 or bool((offsets[1:] < offsets[:-1]).any())):
            raise ValueError("offsets must start at 0, be non-decreasing and end inside ids")
    else:
        raise ValueError("ids must be 1-D (with offsets) or 2-D (padded)")
    n_in = int(offsets[-1]) if n else 0
    n_rows, n_frags, _ = _synced(torch, dev, core.blocks_ids_device_raw, ids.data_ptr(), offsets.data_ptr(), n, n_in, L, m, pad, t)
    return _take_blocks(torch, core, dev, n_rows, n_frags, L)


def blocks_flush_tensor(bpe, pad_id=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    f, L, _ = core.blocks_open()
    pad_id = _pad_id(bpe, f > 0, pad_id)
    n_rows, n_frags, _ = _synced(torch, dev, core.blocks_flush_raw, 0 if pad_id is None else int(pad_id))
    return _take_blocks(torch, core, dev, n_rows, n_frags, L if n_rows else max(L, 1))


# ---- batches by length under a token budget (include/yttm_mi355x.h "Batches by length") ---------------------------------------------------------
class Batches:
    """order int32 [n] (the kept sentences by (length, index), then the left-out ones), batch_first int64 [n_batches + 1], n_kept; after a gather
    widths int32 [n_batches], batch_off int64 [n_batches + 1], ids int32 [n_elems].  len(b): the batches; b[k] = (sentence indices, matrix), the
    matrix a view of ids."""

    def __init__(self, order, batch_first, n_kept, widths=None, batch_off=None, ids=None):
        self.order, self.batch_first, self.n_kept, self.widths, self.batch_off, self.ids = order, batch_first, n_kept, widths, batch_off, ids
        self._first = self._off = self._w = None

    def __len__(self):
        return self.batch_first.numel() - 1

    def __getitem__(self, k):
        n = len(self)
        if not -n <= k < n:
            raise IndexError("batch %d of %d" % (k, n))
        k %= n
        if self._first is None:  # (one download of the three small arrays, at the first index)
            self._first = self.batch_first.tolist()
            self._off = self.batch_off.tolist() if self.batch_off is not None else None
            self._w = self.widths.tolist() if self.widths is not None else None
        a, b = self._first[k], self._first[k + 1]
        sentences = self.order[a:b]
        if self.ids is None:
            return sentences, None
        return sentences, self.ids[self._off[k]:self._off[k + 1]].view(b - a, self._w[k])

    def __iter__(self):
        return (self[k] for k in range(len(self)))


def _take_batches(torch, core, dev, n, n_kept, n_batches, n_elems):
    """the batches slot as tensors that torch owns"""
    order = torch.empty(n, dtype=torch.int32, device=dev)
    first = torch.zeros(n_batches + 1, dtype=torch.int64, device=dev)
    if n_elems is None:
        _synced(torch, dev, core.copy_batches_device, order.data_ptr(), first.data_ptr(), None, None, None, n, n_batches, 0)
        return Batches(order, first, n_kept)
    widths = torch.empty(n_batches, dtype=torch.int32, device=dev)
    off = torch.zeros(n_batches + 1, dtype=torch.int64, device=dev)
    out = torch.empty(n_elems, dtype=torch.int32, device=dev)
    _synced(torch, dev, core.copy_batches_device, order.data_ptr(), first.data_ptr(), widths.data_ptr(), off.data_ptr(), out.data_ptr(), n, n_batches, n_elems)
    return Batches(order, first, n_kept, widths, off, out)


def _pending_batches(torch, bpe, core, dev, n, max_tokens, max_sentences, min_len, max_len, left_pad, pad_id):
    pad_id = _pad_id(bpe, True, pad_id)
    core.pending_n_sent = n
    n_kept, n_batches, _ = core.batches_plan_device_raw(n, max_tokens, max_sentences, min_len, max_len)
    n_elems, _ = core.batches_gather_device_raw(n, int(pad_id), left_pad)
    return _take_batches(torch, core, dev, n, n_kept, n_batches, n_elems)


def encode_batches_tensor(bpe, sentences, max_tokens, max_sentences=0, min_len=0, max_len=0, left_pad=False, bos=False, eos=False, reverse=False,
                          dropout_prob=0, pad_id=None, device=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, device)
    _check_dropout(dropout_prob)
    _pad_id(bpe, True, pad_id)
    d_bytes, d_off, n, total, longest_in = _sentences_on(torch, sentences, dev)
    _synced(torch, dev, core.encode_device_raw, d_bytes.data_ptr(), d_off.data_ptr(), n, total, longest_in, bos, eos, reverse, dropout_prob)
    return _pending_batches(torch, bpe, core, dev, n, max_tokens, max_sentences, min_len, max_len, left_pad, pad_id)


def encode_text_batches_tensor(bpe, text, max_tokens, max_sentences=0, min_len=0, max_len=0, left_pad=False, bos=False, eos=False, reverse=False,
                               dropout_prob=0, pad_id=None):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    _check_dropout(dropout_prob)
    _pad_id(bpe, True, pad_id)
    d_text, n_bytes = _text_on(torch, text, dev)
    n, _, _ = _synced(torch, dev, core.encode_text_device_raw, d_text.data_ptr(), n_bytes, bos, eos, reverse, dropout_prob)
    return _pending_batches(torch, bpe, core, dev, n, max_tokens, max_sentences, min_len, max_len, left_pad, pad_id)


def batches_plan_tensor(bpe, lengths, max_tokens, max_sentences=0, min_len=0, max_len=0):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    if not hasattr(lengths, "data_ptr") or lengths.dtype != torch.int32 or lengths.dim() != 1:
        raise ValueError("lengths must be a 1-D int32 tensor")
    _check_on(lengths, dev, "lengths")
    lengths = lengths.contiguous()
    n = lengths.numel()
    n_kept, n_batches, _ = _synced(torch, dev, core.batches_plan_lengths_device_raw, lengths.data_ptr(), n, max_tokens, max_sentences, min_len, max_len)
    return _take_batches(torch, core, dev, n, n_kept, n_batches, None)


def batches_gather_tensor(bpe, ids, lengths=None, offsets=None, pad_id=None, left_pad=False):
    torch = _torch()
    core = bpe.bpe_cython
    dev = _device_of(bpe, None)
    pad_id = _pad_id(bpe, True, pad_id)
    if not hasattr(ids, "data_ptr") or ids.dtype != torch.int32:
        raise ValueError("ids must be an int32 tensor")
    _check_on(ids, dev, "ids")
    if ids.dim() == 2:
        if offsets is not None:
            raise ValueError("offsets go with 1-D ids; a 2-D matrix takes lengths")
        n, w = ids.shape
        if lengths is None:
            lens = torch.full((n,), w, dtype=torch.int64, device=dev)
        else:
            _check_on(lengths, dev, "lengths")
            if lengths.dim() != 1 or lengths.numel() != n:
                raise ValueError("lengths must have one entry per row")
            lens = lengths.to(torch.int64).clamp(0, w)
        keep = torch.arange(w, device=dev).unsqueeze(0) < lens.unsqueeze(1)  # the rows' ids back to back (the library's pass takes the ragged form)
        ids = ids[keep].contiguous()
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
    elif ids.dim() == 1:
        if offsets is None or lengths is not None:
            raise ValueError("1-D ids take offsets [n + 1] (and no lengths)")
        offsets = _offsets_u64(torch, offsets, dev)
        ids = ids.contiguous()
        n = offsets.numel() - 1
        if n < 0:
            raise ValueError("offsets must have at least one entry")
        if n and (int(offsets[-1]) > ids.numel() or int(offsets[0]) != 0 or bool((offsets[1:] < offsets[:-1]).any())):
            raise ValueError("offsets must start at 0, be non-decreasing and end inside ids")
    else:
        raise ValueError("ids must be 1-D (with offsets) or 2-D (padded)")
    n_in = int(offsets[-1]) if n else 0
    plan = getattr(core, "batches_last_plan", None)
    if plan is None:
        raise ValueError("batches_gather_tensor: no plan (batches_plan_tensor or encode_batches_tensor first)")
    n_elems, _ = _synced(torch, dev, core.batches_gather_ids_device_raw, ids.data_ptr(), offsets.data_ptr(), n, n_in, int(pad_id), left_pad)
    _, n_kept, n_batches = plan
    return _take_batches(torch, core, dev, n, n_kept, n_batches, n_elems)
