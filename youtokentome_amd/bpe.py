"""Drop-in mirror of `youtokentome.BPE` / `youtokentome.OutputType` (reference: youtokentome/youtokentome.py:6-99) and
of the Cython class it wraps (`_youtokentome_cython.BPE`, youtokentome/cpp/yttm.pyx:51-182), on top of the MI355X C ABI
(include/yttm_mi355x.h).  Same names, argument meaning, return shapes and error behaviour (ValueError / TypeError)."""
import ctypes as C
import os
from collections.abc import Collection
from enum import Enum
from typing import List, Optional, Union

import numpy as np

from . import _lib

try:  # csrc/pyapi.c, built next to the HIP library; without it the list API marshals in Python (slower, same results)
    from . import _yttm_pyapi as _pyapi
except ImportError:  # pragma: no cover
    _pyapi = None


class OutputType(Enum):  # youtokentome.py:6-8
    ID = 1
    SUBWORD = 2


def _err():
    return C.create_string_buffer(_lib.ERRLEN)


def _check_dropout(dropout_prob):  # yttm.pyx:92-93
    if dropout_prob < 0 or dropout_prob > 1:
        raise ValueError("dropout_prob value must be in the range [0, 1]. Current value of dropout_prob = " + str(dropout_prob))


def _pack(sentences):
    """list[str] -> (utf-8 blob, uint64 offsets[n+1])  (the `.encode()` per sentence of yttm.pyx:103)"""
    offs = np.zeros(len(sentences) + 1, dtype=np.uint64)
    if not sentences:
        return b"", offs
    blob = "".join(sentences).encode()
    nchar = np.fromiter(map(len, sentences), dtype=np.int64, count=len(sentences))
    if int(nchar.sum()) == len(blob):  # one byte per char everywhere: the byte offsets are the char offsets, no per-sentence encode
        np.cumsum(nchar, out=offs[1:])
        return blob, offs
    enc = [s.encode() for s in sentences]
    np.cumsum(np.fromiter(map(len, enc), dtype=np.int64, count=len(enc)), out=offs[1:])
    return b"".join(enc), offs


def _take(ptr, n, ctype, dtype):
    L = _lib.load()
    n = int(n)
    arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(max(n, 1),))[:n].astype(dtype, copy=True)
    L.yttm_free(C.cast(ptr, C.c_void_p))
    return arr


class _Malloced:
    """a malloc'ed result of the library as the base of a numpy array: released with yttm_free when the last view of it goes"""

    def __init__(self, ptr, n, dtype):
        self._addr = C.cast(ptr, C.c_void_p).value
        self.__array_interface__ = {"shape": (int(n),), "typestr": np.dtype(dtype).str, "data": (self._addr, False), "version": 3}

    def __del__(self):
        if self._addr:
            _lib.load().yttm_free(C.c_void_p(self._addr))
            self._addr = None


def _adopt(ptr, n, dtype):
    """the same without the copy of _take (a file's ids are gigabytes)"""
    owner = _Malloced(ptr, n, dtype)
    return np.asarray(owner) if n else np.empty(0, dtype)


class _Core:
    """`_youtokentome_cython.BPE` (yttm.pyx:51-182)."""

    def __init__(self, model_path, n_threads=-1, device=0):
        L = _lib.load()
        h = C.c_void_p()
        err = _err()
        rc = L.yttm_encoder_create(model_path.encode(), n_threads, device, C.byref(h), err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode())  # yttm.pyx:61-62
        self._h = h
        self.device = device

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.load().yttm_encoder_destroy(h)
            self._h = None

    @staticmethod
    def train(data, model, vocab_size, coverage=1.0, n_threads=-1, pad_id=0, unk_id=1, bos_id=2, eos_id=3):
        err = _err()
        rc = _lib.load().yttm_train_bpe(data.encode(), model.encode(), vocab_size, coverage, n_threads, pad_id, unk_id,
                                        bos_id, eos_id, err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode())  # yttm.pyx:84-85

    # ---- word cache of the batch encoder (include/yttm_mi355x.h): 0 off, 1 whenever possible, 2 (default) from min_bytes up
    def set_cache(self, mode, min_bytes=8 << 20):
        _lib.load().yttm_encoder_set_cache(self._h, int(mode), int(min_bytes))

    def cache_words(self):
        return int(_lib.load().yttm_encode_cache_words(self._h))

    # ---- encode under a restricted vocabulary (include/yttm_mi355x.h): a mask of allowed ids; tokens outside it are split back into smaller pieces
    def set_vocabulary(self, allowed=None):
        """allowed: a sequence of vocab_size() truth values, or None to clear the vocabulary -> (allowed ids, ids that split, longest expansion)"""
        info, err = (C.c_uint64 * 3)(), _err()
        if allowed is None:
            self._check(_lib.load().yttm_encoder_set_vocabulary(self._h, None, 0, info, err, _lib.ERRLEN), err)
        else:
            mask = np.ascontiguousarray(np.asarray(allowed) != 0, dtype=np.uint8)
            if mask.ndim != 1:
                raise ValueError("allowed must be one-dimensional")
            self._check(_lib.load().yttm_encoder_set_vocabulary(self._h, mask.ctypes.data_as(_lib.u8p), len(mask), info, err, _lib.ERRLEN), err)
        self._vocabulary_info = tuple(int(v) for v in info)
        return self._vocabulary_info

    def vocabulary_info(self):
        return getattr(self, "_vocabulary_info", (0, 0, 0))

    def vocabulary_stats(self):
        """-> (restricted calls, calls where nothing split, ids in, ids out)"""
        out = (C.c_uint64 * 4)()
        _lib.load().yttm_encoder_vocabulary_stats(self._h, out)
        return tuple(int(v) for v in out)

    def restrict_ids_device_raw(self, d_ids, d_offsets, n_sent, n_ids, reverse=False):
        """-> (n_out, kernel_ms); the restricted ids are pending as after encode_device_raw"""
        n, ms, err = C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_restrict_ids_device(self._h, C.c_void_p(d_ids), C.c_void_p(d_offsets), n_sent, n_ids, int(bool(reverse)), C.byref(n),
                                                         C.byref(ms), err, _lib.ERRLEN), err)
        return n.value, ms.value

    # ---- byte fallback (include/yttm_mi355x.h "Byte fallback"): the bytes of an unknown run as the ids vocab_size() + b in place of one <UNK>
    def set_byte_fallback(self, on=True):
        err = _err()
        self._check(_lib.load().yttm_encoder_set_byte_fallback(self._h, int(bool(on)), err, _lib.ERRLEN), err)

    def byte_fallback(self):
        return bool(_lib.load().yttm_encoder_byte_fallback(self._h))

    def id_bound(self):
        """the ids the decode, the names and the counts know: vocab_size(), with the byte fallback on 256 more; with n added tokens
        vocab_size() + 256 + n whether the byte fallback is on or not"""
        n = self.n_added_tokens()
        return self.vocab_size() + 256 + n if n else self.vocab_size() + (256 if self.byte_fallback() else 0)

    def byte_fallback_stats(self):
        """-> (calls of the pass, calls whose write pass was skipped, ids in, ids out)"""
        out = (C.c_uint64 * 4)()
        _lib.load().yttm_encoder_byte_fallback_stats(self._h, out)
        return tuple(int(v) for v in out)

    def byte_fallback_ids_device_raw(self, d_ids, d_id_offsets, d_bytes, d_text_offsets, n_sent, n_ids, total_bytes, reverse=False):
        """-> (n_out, kernel_ms); the ids are pending as after encode_device_raw"""
        n, ms, err = C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_byte_fallback_ids_device(self._h, C.c_void_p(d_ids), C.c_void_p(d_id_offsets), C.c_void_p(d_bytes), C.c_void_p(d_text_offsets),
                                                              n_sent, n_ids, total_bytes, int(bool(reverse)), C.byref(n), C.byref(ms), err, _lib.ERRLEN), err)
        return n.value, ms.value

    # ---- added tokens (include/yttm_mi355x.h "Added tokens"): literal strings that are one id each, vocab_size() + 256 + k, and never split
    def set_added_tokens(self, tokens=None):
        """tokens: a sequence of str or bytes in the order of their ids, or None to clear the setting"""
        err = _err()
        if tokens is None:
            self._check(_lib.load().yttm_encoder_set_added_tokens(self._h, None, None, 0, err, _lib.ERRLEN), err)
            return
        if isinstance(tokens, (str, bytes)):
            raise TypeError("tokens must be a sequence of strings, not one string")
        raw = [t.encode() if isinstance(t, str) else bytes(t) for t in tokens]
        off = np.zeros(len(raw) + 1, np.uint64)
        off[1:] = np.cumsum([len(t) for t in raw], dtype=np.uint64)
        blob = np.frombuffer(b"".join(raw) + b"\0", np.uint8)  # (never empty: an empty token is the library's error, with its message)
        self._check(_lib.load().yttm_encoder_set_added_tokens(self._h, blob.ctypes.data_as(_lib.u8p), off.ctypes.data_as(_lib.u64p), len(raw), err,
                                                              _lib.ERRLEN), err)

    def added_tokens_raw(self):
        """the tokens as bytes, in the order of their ids ([] while nothing is set)"""
        L = _lib.load()
        blob_p, off, n = C.c_void_p(), _lib.u64p(), C.c_uint64()
        L.yttm_encoder_added_tokens(self._h, C.byref(blob_p), C.byref(off), C.byref(n))
        oo = _take(off, n.value + 1, C.c_uint64, np.uint64)
        raw = C.string_at(blob_p, int(oo[-1]))
        L.yttm_free(blob_p)
        return [raw[int(oo[i]):int(oo[i + 1])] for i in range(n.value)]

    def n_added_tokens(self):
        L = _lib.load()
        blob_p, off, n = C.c_void_p(), _lib.u64p(), C.c_uint64()
        L.yttm_encoder_added_tokens(self._h, C.byref(blob_p), C.byref(off), C.byref(n))
        L.yttm_free(blob_p)
        L.yttm_free(C.cast(off, C.c_void_p))
        return int(n.value)

    def added_tokens_stats(self):
        """-> (calls with the setting on, calls without a match, matches, sub-sentences encoded)"""
        out = (C.c_uint64 * 4)()
        _lib.load().yttm_encoder_added_tokens_stats(self._h, out)
        return tuple(int(v) for v in out)

    def added_split_device_raw(self, d_bytes, d_offsets, n_sent, total_bytes):
        """-> (n_sub, n_matches, kernel_ms); the three arrays stay in the encoder until fetch_added_split / copy_added_split takes them"""
        ns, nm, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_added_split_device(self._h, C.c_void_p(d_bytes), C.c_void_p(d_offsets), n_sent, total_bytes, C.byref(ns), C.byref(nm),
                                                        C.byref(ms), err, _lib.ERRLEN), err)
        return ns.value, nm.value, ms.value

    def fetch_added_split(self, n_sent, n_sub):
        """-> (sub_first uint64 [n_sent + 1], sub_offsets uint64 [n_sub + 1], tok int32 [n_sub])"""
        first, off, tok, err = np.zeros(n_sent + 1, np.uint64), np.zeros(n_sub + 1, np.uint64), np.zeros(n_sub, np.int32), _err()
        self._check(_lib.load().yttm_added_split_fetch(self._h, first.ctypes.data_as(_lib.u64p), off.ctypes.data_as(_lib.u64p), tok.ctypes.data_as(_lib.i32p),
                                                       n_sent, n_sub, err, _lib.ERRLEN), err)
        return first, off, tok

    def copy_added_split(self, d_first, d_off, d_tok, n_sent, n_sub):
        err = _err()
        self._check(_lib.load().yttm_added_split_copy_device(self._h, C.c_void_p(d_first), C.c_void_p(d_off), C.c_void_p(d_tok), n_sent, n_sub, err,
                                                             _lib.ERRLEN), err)

    # ---- packed fast path: bytes + offsets -> numpy ids + offsets
    def encode_packed(self, blob: bytes, offsets, bos=False, eos=False, reverse=False, dropout_prob=0.0):
        L = _lib.load()
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        ids, off = _lib.i32p(), _lib.u64p()
        err = _err()
        rc = L.yttm_encode_as_ids(self._h, blob, offsets.ctypes.data_as(_lib.u64p), n, int(bos), int(eos), int(reverse),
                                  float(dropout_prob), C.byref(ids), C.byref(off), err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode())
        off_a = _take(off, n + 1, C.c_uint64, np.uint64)
        ids_a = _take(ids, int(off_a[-1]), C.c_int32, np.int32)
        return ids_a, off_a

    # ---- raw device layer (include/yttm_mi355x.h): integer device pointers and sizes, no framework.  youtokentome_amd/tensor.py puts torch
    # tensors on top; the emulator tests pass numpy arrays (there host pointers are device pointers).  The caller makes its inputs visible
    # first; every call returns after the encoder's stream has synchronised.
    def _check(self, rc, err):
        if rc != 0:
            raise ValueError(err.value.decode())

    def encode_device_raw(self, d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos=False, eos=False, reverse=False, dropout_prob=0.0):
        """-> (n_ids, kernel_ms); the ids stay in the encoder until copy_encode_* / yttm_encode_fetch takes them"""
        n, ms, err = C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_encode_device(self._h, C.c_void_p(d_bytes), C.c_void_p(d_offsets), n_sent, total_bytes, max_sentence_bytes, int(bos),
                                                   int(eos), int(reverse), float(dropout_prob), C.byref(n), C.byref(ms), err, _lib.ERRLEN), err)
        return n.value, ms.value

    def copy_encode_device(self, d_ids, d_out_offsets, n_sent):
        err = _err()
        self._check(_lib.load().yttm_encode_copy_device(self._h, C.c_void_p(d_ids), C.c_void_p(d_out_offsets), n_sent, err, _lib.ERRLEN), err)

    def encode_longest(self, n_sent):
        """longest row of the pending encode result (asks for a matrix of width 0: nothing is written when a row is longer)"""
        longest, err = C.c_uint64(), _err()
        _lib.load().yttm_encode_copy_padded(self._h, None, None, n_sent, 0, 0, C.byref(longest), err, _lib.ERRLEN)
        return longest.value

    def copy_encode_padded(self, d_matrix, d_lengths, n_sent, width, pad_value):
        """-> longest row; ValueError when width is smaller"""
        longest, err = C.c_uint64(), _err()
        self._check(_lib.load().yttm_encode_copy_padded(self._h, C.c_void_p(d_matrix), C.c_void_p(d_lengths), n_sent, width, int(pad_value),
                                                        C.byref(longest), err, _lib.ERRLEN), err)
        return longest.value

    @staticmethod
    def _ignore(ignore_ids):
        ign = np.ascontiguousarray(sorted(set(int(i) for i in (ignore_ids or ()))), dtype=np.int32)
        return ign, ign.ctypes.data_as(_lib.i32p), len(ign)

    def decode_device_raw(self, d_ids, d_offsets, n_sent, n_ids, ignore_ids=None):
        """-> (n_bytes, kernel_ms); the text stays in the encoder until fetch_decode / copy_decode_device takes it"""
        ign, ign_p, n_ign = self._ignore(ignore_ids)
        n, ms, err = C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_decode_device(self._h, C.c_void_p(d_ids), C.c_void_p(d_offsets), n_sent, n_ids, ign_p, n_ign, C.byref(n), C.byref(ms),
                                                   err, _lib.ERRLEN), err)
        return n.value, ms.value

    def decode_device_padded_raw(self, d_ids, n_sent, width, row_stride, d_lengths=None, ignore_ids=None):
        ign, ign_p, n_ign = self._ignore(ignore_ids)
        n, ms, err = C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_decode_device_padded(self._h, C.c_void_p(d_ids), n_sent, width, row_stride, C.c_void_p(d_lengths), ign_p, n_ign,
                                                          C.byref(n), C.byref(ms), err, _lib.ERRLEN), err)
        return n.value, ms.value

    def fetch_decode(self, n_sent, n_bytes):
        """-> (uint8 bytes[n_bytes], uint64 offsets[n_sent + 1]) on the host"""
        raw, off, err = np.empty(max(int(n_bytes), 1), np.uint8), np.zeros(n_sent + 1, np.uint64), _err()
        self._check(_lib.load().yttm_decode_fetch(self._h, C.c_void_p(raw.ctypes.data), off.ctypes.data_as(_lib.u64p), n_sent, err, _lib.ERRLEN), err)
        return raw[:int(n_bytes)], off

    def copy_decode_device(self, d_bytes, d_out_offsets, n_sent):
        err = _err()
        self._check(_lib.load().yttm_decode_copy_device(self._h, C.c_void_p(d_bytes), C.c_void_p(d_out_offsets), n_sent, err, _lib.ERRLEN), err)

    # ---- text that is not cut into sentences yet (include/yttm_mi355x.h): the lines are found on the device
    def lines_device_raw(self, d_text, n_bytes):
        """-> (n_lines, longest, kernel_ms); the offsets stay in the encoder until copy_lines_device / fetch_lines takes them"""
        n, longest, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_lines_device(self._h, C.c_void_p(d_text), n_bytes, C.byref(n), C.byref(longest), C.byref(ms), err, _lib.ERRLEN), err)
        return n.value, longest.value, ms.value

    def copy_lines_device(self, d_offsets, n_lines):
        err = _err()
        self._check(_lib.load().yttm_lines_copy_device(self._h, C.c_void_p(d_offsets), n_lines, err, _lib.ERRLEN), err)

    def fetch_lines(self, n_lines):
        """-> uint64 offsets[n_lines + 1] on the host"""
        off, err = np.zeros(n_lines + 1, np.uint64), _err()
        self._check(_lib.load().yttm_lines_fetch(self._h, off.ctypes.data_as(_lib.u64p), n_lines, err, _lib.ERRLEN), err)
        return off

    def encode_text_device_raw(self, d_text, n_bytes, bos=False, eos=False, reverse=False, dropout_prob=0.0):
        """-> (n_lines, n_ids, kernel_ms); the ids are pending as after encode_device_raw with n_sent = n_lines"""
        nl, ni, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_encode_text_device(self._h, C.c_void_p(d_text), n_bytes, int(bos), int(eos), int(reverse), float(dropout_prob),
                                                        C.byref(nl), C.byref(ni), C.byref(ms), err, _lib.ERRLEN), err)
        return nl.value, ni.value, ms.value

    def fetch_encode(self, n_sent, n_ids):
        """the pending encode result -> (int32 ids[n_ids], uint64 offsets[n_sent + 1]) on the host"""
        ids, off, err = np.empty(max(int(n_ids), 1), np.int32), np.zeros(n_sent + 1, np.uint64), _err()
        self._check(_lib.load().yttm_encode_fetch(self._h, ids.ctypes.data_as(_lib.i32p), off.ctypes.data_as(_lib.u64p), n_sent, err, _lib.ERRLEN), err)
        return ids[:int(n_ids)], off

    def encode_file(self, path, out=None, bos=False, eos=False, reverse=False, dropout_prob=0.0, chunk_bytes=None, report=False):
        """a text file -> (int32 ids, uint64 offsets[n_lines + 1]), or with out=PREFIX the files PREFIX.ids / PREFIX.off and (n_lines, n_ids);
        report=True appends the call's report (a dict) to the result"""
        _check_dropout(dropout_prob)
        L = _lib.load()
        ids, off, nl, ni, err = _lib.i32p(), _lib.u64p(), C.c_uint64(), C.c_uint64(), _err()
        rep = C.create_string_buffer(1024)
        rc = L.yttm_encode_file(self._h, os.fsencode(path), None if out is None else os.fsencode(out), int(bos), int(eos), int(reverse), float(dropout_prob),
                                int(chunk_bytes or 0), None if out is not None else C.byref(ids), None if out is not None else C.byref(off),
                                C.byref(nl), C.byref(ni), rep, len(rep), err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode(errors="replace"))
        if out is not None:
            res = (nl.value, ni.value)
        else:
            res = (_adopt(ids, ni.value, np.int32), _adopt(off, nl.value + 1, np.uint64))
        if report:
            import json
            res += (json.loads(rep.value.decode()),)
        return res

    # ---- SUBWORD output on the device (include/yttm_mi355x.h): the text stays in the encoder until fetch_decode / copy_decode_device takes it
    def subword_device_raw(self, d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos=False, eos=False, reverse=False, dropout_prob=0.0):
        """-> (n_ids, n_text_bytes, kernel_ms); the ids are pending as after encode_device_raw, the text replaces a pending decode result"""
        ni, nt, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_subword_device(self._h, C.c_void_p(d_bytes), C.c_void_p(d_offsets), n_sent, total_bytes, max_sentence_bytes, int(bos),
                                                    int(eos), int(reverse), float(dropout_prob), C.byref(ni), C.byref(nt), C.byref(ms), err, _lib.ERRLEN), err)
        return ni.value, nt.value, ms.value

    def subword_text_device_raw(self, d_text, n_bytes, bos=False, eos=False, reverse=False, dropout_prob=0.0):
        """-> (n_lines, n_ids, n_text_bytes, kernel_ms)"""
        nl, ni, nt, ms, err = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_subword_text_device(self._h, C.c_void_p(d_text), n_bytes, int(bos), int(eos), int(reverse), float(dropout_prob),
                                                         C.byref(nl), C.byref(ni), C.byref(nt), C.byref(ms), err, _lib.ERRLEN), err)
        return nl.value, ni.value, nt.value, ms.value

    def _file_to_text(self, entry, path, out, args, chunk_bytes, report):
        """one of the library's file-to-text entries (`args`: what it takes between the two paths and the piece size) -> (n_lines, n_ids,
        n_text_bytes), or with report=True the call's report (a dict)"""
        nl, ni, nt, err = C.c_uint64(), C.c_uint64(), C.c_uint64(), _err()
        rep = C.create_string_buffer(1024)
        rc = getattr(_lib.load(), entry)(self._h, os.fsencode(path), os.fsencode(out), *args, int(chunk_bytes or 0), C.byref(nl), C.byref(ni), C.byref(nt),
                                         rep, len(rep), err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode(errors="replace"))
        if report:
            import json
            return json.loads(rep.value.decode())
        return nl.value, ni.value, nt.value

    def encode_file_subword(self, path, out, bos=False, eos=False, reverse=False, dropout_prob=0.0, chunk_bytes=None, report=False):
        """a text file -> the text file `yttm encode --output_type subword` prints for it, written to `out`: (n_lines, n_ids, n_text_bytes), or with
        report=True the call's report (a dict)"""
        _check_dropout(dropout_prob)
        if out is None:
            raise ValueError("encode_file with output_type SUBWORD needs out, the path of the text file to write")
        return self._file_to_text("yttm_encode_file_subword", path, out, (int(bos), int(eos), int(reverse), float(dropout_prob)), chunk_bytes, report)

    # ---- byte spans on the device (include/yttm_mi355x.h): the spans stay in the encoder, beside the ids they belong to, until an encode replaces those
    def spans_device_raw(self, d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos=False, eos=False, reverse=False, dropout_prob=0.0):
        """-> (n_ids, kernel_ms); the ids are pending as after encode_device_raw, the spans until copy_spans_* / fetch_spans takes them"""
        ni, ms, err = C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_spans_device(self._h, C.c_void_p(d_bytes), C.c_void_p(d_offsets), n_sent, total_bytes, max_sentence_bytes, int(bos),
                                                  int(eos), int(reverse), float(dropout_prob), C.byref(ni), C.byref(ms), err, _lib.ERRLEN), err)
        return ni.value, ms.value

    def spans_text_device_raw(self, d_text, n_bytes, bos=False, eos=False, reverse=False, dropout_prob=0.0):
        """-> (n_lines, n_ids, kernel_ms)"""
        nl, ni, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_spans_text_device(self._h, C.c_void_p(d_text), n_bytes, int(bos), int(eos), int(reverse), float(dropout_prob),
                                                       C.byref(nl), C.byref(ni), C.byref(ms), err, _lib.ERRLEN), err)
        return nl.value, ni.value, ms.value

    def fetch_spans(self, n_sent, n_ids):
        """the pending spans -> np.uint32 [n_ids, 2]"""
        spans, err = np.zeros((int(n_ids), 2), np.uint32), _err()
        self._check(_lib.load().yttm_spans_fetch(self._h, spans.ctypes.data_as(_lib.u32p), n_sent, err, _lib.ERRLEN), err)
        return spans

    def copy_spans_device(self, d_spans, n_sent):
        err = _err()
        self._check(_lib.load().yttm_spans_copy_device(self._h, C.c_void_p(d_spans), n_sent, err, _lib.ERRLEN), err)

    def copy_spans_padded(self, d_matrix, n_sent, width):
        """-> longest row; ValueError when width is smaller"""
        longest, err = C.c_uint64(), _err()
        self._check(_lib.load().yttm_spans_copy_padded(self._h, C.c_void_p(d_matrix), n_sent, width, C.byref(longest), err, _lib.ERRLEN), err)
        return longest.value

    def encode_packed_spans(self, blob: bytes, offsets, bos=False, eos=False, reverse=False, dropout_prob=0.0):
        """host to host: -> (ids np.int32, offsets np.uint64 [n + 1], spans np.uint32 [n_ids, 2])"""
        L = _lib.load()
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        ids, off, spans = _lib.i32p(), _lib.u64p(), _lib.u32p()
        err = _err()
        rc = L.yttm_encode_as_ids_spans(self._h, blob, offsets.ctypes.data_as(_lib.u64p), n, int(bos), int(eos), int(reverse), float(dropout_prob),
                                        C.byref(ids), C.byref(off), C.byref(spans), err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode())
        off_a = _take(off, n + 1, C.c_uint64, np.uint64)
        ids_a = _take(ids, int(off_a[-1]), C.c_int32, np.int32)
        spans_a = _take(spans, 2 * int(off_a[-1]), C.c_uint32, np.uint32).reshape(-1, 2)
        return ids_a, off_a, spans_a

    # ---- token frequencies on the device (include/yttm_mi355x.h): uint64 counts[n_bins + 1] in a slot of the encoder's own, the last one the ids
    # outside [0, n_bins); n_bins = 0: the vocabulary's size
    def id_counts_device_raw(self, n_sent, n_bins=0, accumulate=False):
        """counts the pending encode result of n_sent sentences -> (n_counted, kernel_ms); the result stays pending"""
        nc, ms, err = C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_id_counts_device(self._h, n_sent, int(n_bins), int(bool(accumulate)), C.byref(nc), C.byref(ms), err, _lib.ERRLEN), err)
        return nc.value, ms.value

    def id_counts_ids_device_raw(self, d_ids, n_ids, n_bins=0, accumulate=False):
        """counts int32 ids[n_ids] in device memory -> kernel_ms"""
        ms, err = C.c_double(), _err()
        self._check(_lib.load().yttm_id_counts_ids_device(self._h, C.c_void_p(d_ids), n_ids, int(n_bins), int(bool(accumulate)), C.byref(ms), err,
                                                          _lib.ERRLEN), err)
        return ms.value

    def fetch_id_counts(self, n_bins=0):
        """the counts -> np.uint64 [n_bins + 1]"""
        counts, err = np.zeros(int(n_bins or self.id_bound()) + 1, np.uint64), _err()
        self._check(_lib.load().yttm_id_counts_fetch(self._h, counts.ctypes.data_as(_lib.u64p), int(n_bins), err, _lib.ERRLEN), err)
        return counts

    def copy_id_counts_device(self, d_counts, n_bins=0):
        err = _err()
        self._check(_lib.load().yttm_id_counts_copy_device(self._h, C.c_void_p(d_counts), int(n_bins), err, _lib.ERRLEN), err)

    def encode_file_counts(self, path, bos=False, eos=False, reverse=False, dropout_prob=0.0, chunk_bytes=None, report=False):
        """a text file -> np.uint64 counts[vocab_size + 1] of its ids (with the byte fallback on: [vocab_size + 256 + 1]; and with report=True the
        call's report, a dict); report["lines"] and report["ids"] are the file's"""
        _check_dropout(dropout_prob)
        counts = np.zeros(self.id_bound() + 1, np.uint64)
        nl, ni, err = C.c_uint64(), C.c_uint64(), _err()
        rep = C.create_string_buffer(1024)
        rc = _lib.load().yttm_encode_file_counts(self._h, os.fsencode(path), int(bos), int(eos), int(reverse), float(dropout_prob), int(chunk_bytes or 0),
                                                 counts.ctypes.data_as(_lib.u64p), C.byref(nl), C.byref(ni), rep, len(rep), err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode(errors="replace"))
        if report:
            import json
            return counts, json.loads(rep.value.decode())
        return counts

    # ---- training blocks on the device (include/yttm_mi355x.h "Training blocks"): rows of exactly seq_len ids in a slot of the encoder's own
    MODES = {"stream": 0, "whole": 1}
    TAILS = {"pad": 0, "keep": 1, "drop": 2}

    def blocks_device_raw(self, n_sent, seq_len, mode=0, pad_value=0, tail=0):
        """packs the pending encode result of n_sent sentences -> (n_rows, n_frags, kernel_ms); the result stays pending"""
        nr, nf, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_blocks_device(self._h, n_sent, int(seq_len), int(mode), int(pad_value), int(tail), C.byref(nr), C.byref(nf), C.byref(ms),
                                                   err, _lib.ERRLEN), err)
        return nr.value, nf.value, ms.value

    def blocks_ids_device_raw(self, d_ids, d_offsets, n_sent, n_ids, seq_len, mode=0, pad_value=0, tail=0):
        """packs int32 ids[n_ids] + uint64 offsets[n_sent + 1] in device memory -> (n_rows, n_frags, kernel_ms)"""
        nr, nf, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_blocks_ids_device(self._h, C.c_void_p(d_ids), C.c_void_p(d_offsets), n_sent, n_ids, int(seq_len), int(mode), int(pad_value),
                                                       int(tail), C.byref(nr), C.byref(nf), C.byref(ms), err, _lib.ERRLEN), err)
        return nr.value, nf.value, ms.value

    def blocks_flush_raw(self, pad_value=0):
        """the open row as a result of 0 or 1 rows -> (n_rows, n_frags, kernel_ms)"""
        nr, nf, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_blocks_flush(self._h, int(pad_value), C.byref(nr), C.byref(nf), C.byref(ms), err, _lib.ERRLEN), err)
        return nr.value, nf.value, ms.value

    def blocks_open(self):
        """(ids in the open row, its seq_len, its mode); zeroes when it is empty"""
        out = (C.c_uint64 * 3)()
        _lib.load().yttm_blocks_open(self._h, out)
        return int(out[0]), int(out[1]), int(out[2])

    def blocks_discard(self):
        _lib.load().yttm_blocks_discard(self._h)

    def fetch_blocks(self, n_rows, n_frags, seq_len):
        """the blocks slot -> (rows, seg, pos [n_rows, seq_len] int32, frags [n_frags, 2] int32, row_frags [n_rows + 1] uint64)"""
        rows, seg, pos = (np.zeros((n_rows, seq_len), np.int32) for _ in range(3))
        frags, row_frags, err = np.zeros((n_frags, 2), np.int32), np.zeros(n_rows + 1, np.uint64), _err()
        self._check(_lib.load().yttm_blocks_fetch(self._h, rows.ctypes.data_as(_lib.i32p), seg.ctypes.data_as(_lib.i32p), pos.ctypes.data_as(_lib.i32p),
                                                  frags.ctypes.data_as(_lib.i32p), row_frags.ctypes.data_as(_lib.u64p), n_rows, n_frags, err, _lib.ERRLEN), err)
        return rows, seg, pos, frags, row_frags

    def copy_blocks_device(self, d_rows, d_seg, d_pos, d_frags, d_row_frags, n_rows, n_frags):
        err = _err()
        self._check(_lib.load().yttm_blocks_copy_device(self._h, C.c_void_p(d_rows), C.c_void_p(d_seg), C.c_void_p(d_pos), C.c_void_p(d_frags),
                                                        C.c_void_p(d_row_frags), n_rows, n_frags, err, _lib.ERRLEN), err)

    def encode_file_blocks(self, path, out, seq_len, mode=0, bos=False, eos=False, reverse=False, dropout_prob=0.0, pad_value=0, tail=0, chunk_bytes=None,
                           report=False):
        """a text file -> OUT.rows (int32 [n_rows, seq_len]) and OUT.frags (uint64 [n_frags, 2]): (n_rows, n_frags, n_lines, n_ids), or with report=True
        the call's report (a dict)"""
        _check_dropout(dropout_prob)
        nr, nf, nl, ni, err = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), _err()
        rep = C.create_string_buffer(1024)
        rc = _lib.load().yttm_encode_file_blocks(self._h, os.fsencode(path), os.fsencode(out), int(bos), int(eos), int(reverse), float(dropout_prob),
                                                 int(chunk_bytes or 0), int(seq_len), int(mode), int(pad_value), int(tail), C.byref(nr), C.byref(nf), C.byref(nl),
                                                 C.byref(ni), rep, len(rep), err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode(errors="replace"))
        if report:
            import json
            return json.loads(rep.value.decode())
        return nr.value, nf.value, nl.value, ni.value

    # ---- batches by length under a token budget (include/yttm_mi355x.h "Batches by length"): the plan and the gathered batches in a slot of the encoder's own
    def batches_plan_device_raw(self, n_sent, max_tokens, max_sentences=0, min_len=0, max_len=0):
        """plans from the pending encode result of n_sent sentences -> (n_kept, n_batches, kernel_ms); the result stays pending"""
        nk, nb, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_batches_plan_device(self._h, n_sent, int(max_tokens), int(max_sentences), int(min_len), int(max_len), C.byref(nk), C.byref(nb),
                                                         C.byref(ms), err, _lib.ERRLEN), err)
        self.batches_last_plan = (n_sent, nk.value, nb.value)  # (the tensor layer sizes a later gather's tensors from it)
        return nk.value, nb.value, ms.value

    def batches_plan_lengths_device_raw(self, d_lengths, n_sent, max_tokens, max_sentences=0, min_len=0, max_len=0):
        """plans from int32 lengths[n_sent] in device memory -> (n_kept, n_batches, kernel_ms)"""
        nk, nb, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_batches_plan_lengths_device(self._h, C.c_void_p(d_lengths), n_sent, int(max_tokens), int(max_sentences), int(min_len),
                                                                 int(max_len), C.byref(nk), C.byref(nb), C.byref(ms), err, _lib.ERRLEN), err)
        self.batches_last_plan = (n_sent, nk.value, nb.value)
        return nk.value, nb.value, ms.value

    def batches_gather_device_raw(self, n_sent, pad_value=0, left_pad=False):
        """the planned batches of the pending encode result -> (n_elems, kernel_ms)"""
        ne, ms, err = C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_batches_gather_device(self._h, n_sent, int(pad_value), int(bool(left_pad)), C.byref(ne), C.byref(ms), err, _lib.ERRLEN), err)
        return ne.value, ms.value

    def batches_gather_ids_device_raw(self, d_ids, d_offsets, n_sent, n_ids, pad_value=0, left_pad=False):
        """the planned batches of int32 ids[n_ids] + uint64 offsets[n_sent + 1] in device memory -> (n_elems, kernel_ms)"""
        ne, ms, err = C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_batches_gather_ids_device(self._h, C.c_void_p(d_ids), C.c_void_p(d_offsets), n_sent, n_ids, int(pad_value), int(bool(left_pad)),
                                                               C.byref(ne), C.byref(ms), err, _lib.ERRLEN), err)
        return ne.value, ms.value

    def fetch_batches(self, n_sent, n_batches, n_elems=None):
        """the batches slot -> (order uint32 [n_sent], batch_first uint64 [n_batches + 1]) and, with n_elems (a gather has run), widths uint32
        [n_batches], batch_off uint64 [n_batches + 1], out int32 [n_elems]"""
        order, first, err = np.zeros(n_sent, np.uint32), np.zeros(n_batches + 1, np.uint64), _err()
        if n_elems is None:
            self._check(_lib.load().yttm_batches_fetch(self._h, order.ctypes.data, first.ctypes.data, None, None, None, n_sent, n_batches, 0, err,
                                                       _lib.ERRLEN), err)
            return order, first
        widths, off, out = np.zeros(n_batches, np.uint32), np.zeros(n_batches + 1, np.uint64), np.zeros(n_elems, np.int32)
        self._check(_lib.load().yttm_batches_fetch(self._h, order.ctypes.data, first.ctypes.data, widths.ctypes.data, off.ctypes.data, out.ctypes.data,
                                                   n_sent, n_batches, n_elems, err, _lib.ERRLEN), err)
        return order, first, widths, off, out

    def copy_batches_device(self, d_order, d_batch_first, d_widths, d_batch_off, d_out, n_sent, n_batches, n_elems):
        err = _err()
        self._check(_lib.load().yttm_batches_copy_device(self._h, C.c_void_p(d_order), C.c_void_p(d_batch_first), C.c_void_p(d_widths), C.c_void_p(d_batch_off),
                                                         C.c_void_p(d_out), n_sent, n_batches, n_elems, err, _lib.ERRLEN), err)

    # ---- decimal id text on the device (include/yttm_mi355x.h): the format `yttm encode --output_type id` prints and `yttm decode` reads
    def ids_parse_device_raw(self, d_text, n_bytes):
        """-> (n_lines, n_ids, kernel_ms); the ids `while (ss >> x)` reads from every line are pending as after encode_device_raw with n_sent = n_lines"""
        nl, ni, ms, err = C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_ids_parse_device(self._h, C.c_void_p(d_text), n_bytes, C.byref(nl), C.byref(ni), C.byref(ms), err, _lib.ERRLEN), err)
        return nl.value, ni.value, ms.value

    def decode_text_device_raw(self, d_text, n_bytes, ignore_ids=None):
        """-> (n_lines, n_ids, n_text_bytes, kernel_ms); the decoded lines, a newline behind each, are pending in the text slot"""
        ign, ign_p, n_ign = self._ignore(ignore_ids)
        nl, ni, nt, ms, err = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_decode_text_device(self._h, C.c_void_p(d_text), n_bytes, ign_p, n_ign, C.byref(nl), C.byref(ni), C.byref(nt), C.byref(ms),
                                                        err, _lib.ERRLEN), err)
        return nl.value, ni.value, nt.value, ms.value

    def idtext_device_raw(self, n_sent):
        """the pending encode result of n_sent sentences as decimal text in the text slot -> (n_text_bytes, kernel_ms)"""
        nt, ms, err = C.c_uint64(), C.c_double(), _err()
        self._check(_lib.load().yttm_idtext_device(self._h, n_sent, C.byref(nt), C.byref(ms), err, _lib.ERRLEN), err)
        return nt.value, ms.value

    def decode_file(self, path, out, ignore_ids=None, chunk_bytes=None, report=False):
        """a text file of decimal ids, one sentence per line -> the text file `yttm decode` prints for it, written to `out`:
        (n_lines, n_ids, n_text_bytes), or with report=True the call's report (a dict)"""
        if out is None:
            raise ValueError("decode_file needs out, the path of the text file to write")
        ign, ign_p, n_ign = self._ignore(ignore_ids)
        return self._file_to_text("yttm_decode_file", path, out, (ign_p, n_ign), chunk_bytes, report)

    def encode_file_idtext(self, path, out, bos=False, eos=False, reverse=False, dropout_prob=0.0, chunk_bytes=None, report=False):
        """a text file -> the text file `yttm encode --output_type id` prints for it, written to `out`: (n_lines, n_ids, n_text_bytes), or with
        report=True the call's report (a dict)"""
        _check_dropout(dropout_prob)
        if out is None:
            raise ValueError("encode_file with id_text=True needs out, the path of the text file to write")
        return self._file_to_text("yttm_encode_file_idtext", path, out, (int(bos), int(eos), int(reverse), float(dropout_prob)), chunk_bytes, report)

    def encode(self, sentences, output_type, bos, eos, reverse, dropout_prob):
        _check_dropout(dropout_prob)
        single = isinstance(sentences, str)
        if single:
            batch = [sentences]
        else:
            assert isinstance(sentences, list) or isinstance(sentences, tuple)
            batch = list(sentences)
        if output_type == "id" and _pyapi is not None:
            # list[str] -> blob + offsets -> yttm_encode_as_ids -> list[list[int]] in C (csrc/pyapi.c: what yttm.pyx:87-109 does in Cython)
            L = _lib.load()
            out = _pyapi.encode_ids(C.cast(L.yttm_encode_as_ids, C.c_void_p).value, C.cast(L.yttm_free, C.c_void_p).value, self._h.value,
                                    batch, bool(bos), bool(eos), bool(reverse), float(dropout_prob))
            return out[0] if single else out
        blob, offs = _pack(batch)
        if output_type == "id":
            ids, off = self.encode_packed(blob, offs, bos, eos, reverse, dropout_prob)
            flat, o = ids.tolist(), off.tolist()  # (slicing a list of ints is several times faster than numpy slice + tolist per sentence)
            out = [flat[o[i]:o[i + 1]] for i in range(len(batch))]
        elif output_type == "subword":
            L = _lib.load()
            blob_p, poff, soff = C.c_void_p(), _lib.u64p(), _lib.u64p()
            npieces = C.c_uint64()
            err = _err()
            rc = L.yttm_encode_as_subwords(self._h, blob, offs.ctypes.data_as(_lib.u64p), len(batch), int(bos), int(eos),
                                           int(reverse), float(dropout_prob), C.byref(blob_p), C.byref(poff),
                                           C.byref(npieces), C.byref(soff), err, _lib.ERRLEN)
            if rc != 0:
                raise ValueError(err.value.decode())
            po = _take(poff, npieces.value + 1, C.c_uint64, np.uint64)
            so = _take(soff, len(batch) + 1, C.c_uint64, np.uint64)
            raw = C.string_at(blob_p, int(po[-1]))
            L.yttm_free(blob_p)
            pieces = [raw[int(po[i]):int(po[i + 1])].decode() for i in range(npieces.value)]
            out = [pieces[int(so[i]):int(so[i + 1])] for i in range(len(batch))]
        else:
            raise ValueError('output_type must be equal to "id" or "subword"')  # yttm.pyx:124
        return out[0] if single else out

    def subword_to_id(self, subword):
        return _lib.load().yttm_subword_to_id(self._h, subword.encode())

    def id_to_subword(self, id):
        L = _lib.load()
        p = C.c_void_p()
        err = _err()
        rc = L.yttm_id_to_subword(self._h, int(id), C.byref(p), err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode())
        s = C.string_at(p).decode()
        L.yttm_free(p)
        return s

    def decode(self, ids, ignore_ids):
        if not isinstance(ids, list):  # yttm.pyx:138-141
            raise TypeError("{} is not a list instance".format(type(ids)))
        if not isinstance(ignore_ids, Collection) and ignore_ids is not None:
            raise TypeError("{} is not a Collection instance".format(type(ignore_ids)))
        if len(ids) > 0 and isinstance(ids[0], int):
            ids = [ids]
        if ignore_ids is None:
            ignore_ids = set()
        L = _lib.load()
        flat = np.ascontiguousarray([t for s in ids for t in s], dtype=np.int32)
        offs = np.zeros(len(ids) + 1, dtype=np.uint64)
        if ids:
            np.cumsum([len(s) for s in ids], out=offs[1:])
        ign = np.ascontiguousarray(sorted(set(int(i) for i in ignore_ids)), dtype=np.int32)
        blob_p, ooff = C.c_void_p(), _lib.u64p()
        err = _err()
        rc = L.yttm_decode(self._h, flat.ctypes.data_as(_lib.i32p), offs.ctypes.data_as(_lib.u64p), len(ids),
                           ign.ctypes.data_as(_lib.i32p), len(ign), C.byref(blob_p), C.byref(ooff), err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode())
        oo = _take(ooff, len(ids) + 1, C.c_uint64, np.uint64)
        raw = C.string_at(blob_p, int(oo[-1]))
        L.yttm_free(blob_p)
        errors = "replace" if self.byte_fallback() else "strict"  # (byte ids the caller made up may form invalid UTF-8)
        return [raw[int(oo[i]):int(oo[i + 1])].decode(errors=errors) for i in range(len(ids))]

    def vocab_size(self):
        return _lib.load().yttm_vocab_size(self._h)

    # ---- the command line's streaming loops (yttm.pyx:167-181): stdin -> stdout inside the library
    def encode_cli(self, output_type, stream, bos, eos, reverse, dropout_prob, in_fd=0, out_fd=1):
        import sys
        sys.stdout.flush()
        err = _err()
        rc = _lib.load().yttm_encode_cli(self._h, output_type.encode(), int(stream), int(bos), int(eos), int(reverse),
                                         float(dropout_prob), in_fd, out_fd, err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode())

    def decode_cli(self, ignore_ids, in_fd=0, out_fd=1):
        import sys
        sys.stdout.flush()
        ign, ign_p, n_ign = self._ignore(ignore_ids)
        err = _err()
        rc = _lib.load().yttm_decode_cli(self._h, ign_p, n_ign, in_fd, out_fd, err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode())

    def vocab_cli(self, verbose, out_fd=1):
        import sys
        sys.stdout.flush()
        err = _err()
        rc = _lib.load().yttm_vocab_cli(self._h, int(verbose), out_fd, err, _lib.ERRLEN)
        if rc != 0:
            raise ValueError(err.value.decode())

    def vocab(self):
        L = _lib.load()
        blob_p, off = C.c_void_p(), _lib.u64p()
        n = C.c_uint64()
        L.yttm_vocabulary(self._h, C.byref(blob_p), C.byref(off), C.byref(n))
        oo = _take(off, n.value + 1, C.c_uint64, np.uint64)
        raw = C.string_at(blob_p, int(oo[-1]))
        L.yttm_free(blob_p)
        return [raw[int(oo[i]):int(oo[i + 1])].decode() for i in range(n.value)]


class BPE:
    """youtokentome.BPE (youtokentome.py:11-99)."""

    def __init__(self, model: str, n_threads: int = -1):
        self.model = model
        self.n_threads = n_threads
        self.bpe_cython = _Core(model_path=model, n_threads=n_threads)

    @staticmethod
    def train(data: str, model: str, vocab_size: int, coverage: float = 1.0, n_threads: int = -1, pad_id: int = 0,
              unk_id: int = 1, bos_id: int = 2, eos_id: int = 3) -> "BPE":
        _Core.train(data=data, model=model, vocab_size=vocab_size, n_threads=n_threads, coverage=coverage, pad_id=pad_id,
                    unk_id=unk_id, bos_id=bos_id, eos_id=eos_id)
        return BPE(model=model, n_threads=n_threads)

    def encode(self, sentences: List[str], output_type: OutputType = OutputType.ID, bos: bool = False, eos: bool = False,
               reverse: bool = False, dropout_prob: float = 0) -> Union[List[List[int]], List[List[str]]]:
        if not isinstance(output_type, OutputType):
            raise TypeError("parameter output_type must be youtokentome.OutputType, not %s}" % str(type(output_type)))
        output_type_str = "id" if output_type == OutputType.ID else "subword"
        return self.bpe_cython.encode(sentences=sentences, output_type=output_type_str, bos=bos, eos=eos, reverse=reverse,
                                      dropout_prob=dropout_prob)

    def vocab_size(self) -> int:
        return self.bpe_cython.vocab_size()

    def vocab(self) -> List[str]:
        return self.bpe_cython.vocab()

    def subword_to_id(self, subword: str) -> int:
        return self.bpe_cython.subword_to_id(subword)

    def id_to_subword(self, id: int) -> str:
        return self.bpe_cython.id_to_subword(id)

    def decode(self, ids: Union[List[int], List[List[int]]], ignore_ids: Optional[Collection] = None) -> List[str]:
        return self.bpe_cython.decode(ids, ignore_ids)

    # ---- device tensors in, device tensors out (youtokentome_amd/tensor.py; the reference has no counterpart)
    def encode_tensor(self, sentences, bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0, padded: bool = True,
                      width: Optional[int] = None, pad_id: Optional[int] = None, device=None):
        from . import tensor
        return tensor.encode_tensor(self, sentences, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, padded=padded, width=width,
                                    pad_id=pad_id, device=device)

    def encode_text_tensor(self, text, bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0, padded: bool = True,
                           width: Optional[int] = None, pad_id: Optional[int] = None):
        """`text`: a 1-D uint8 tensor on the encoder's device, or bytes / bytearray / memoryview (uploaded); one sentence per line.  Returns what
        encode_tensor returns."""
        from . import tensor
        return tensor.encode_text_tensor(self, text, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, padded=padded, width=width, pad_id=pad_id)

    def text_lines_tensor(self, text):
        """the lines of `text` as an int64 offsets tensor [n_lines + 1] on the device (line i = text[off[i]:off[i + 1]], its newline included)"""
        from . import tensor
        return tensor.text_lines_tensor(self, text)

    def encode_file(self, path, out: Optional[str] = None, bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0,
                    chunk_bytes: Optional[int] = None, output_type: OutputType = OutputType.ID, report: bool = False, id_text: bool = False):
        """A text file, one sentence per line -> (ids np.int32, offsets np.uint64 [n_lines + 1]); with out=PREFIX the raw little-endian files
        PREFIX.ids (int32) and PREFIX.off (uint64) are written instead and (n_lines, n_ids) is returned.  Needs no torch.
        output_type=OutputType.SUBWORD: `out` is required and is the path of a text file, written as `yttm encode --output_type subword` prints it
        (every piece followed by a space, a newline per sentence); returns (n_lines, n_ids, n_text_bytes).  report=True: the call's report (a dict)
        is appended to the ID result, and is the SUBWORD result.
        output_type=OutputType.ID with id_text=True: `out` is required and is the path of a text file, written as `yttm encode --output_type id`
        prints it (every id in decimal followed by a space, a newline per sentence); returns (n_lines, n_ids, n_text_bytes), or the report."""
        if not isinstance(output_type, OutputType):
            raise TypeError("parameter output_type must be youtokentome.OutputType, not %s}" % str(type(output_type)))
        if id_text:
            if output_type != OutputType.ID:
                raise ValueError("id_text goes with output_type ID")
            return self.bpe_cython.encode_file_idtext(path, out, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, chunk_bytes=chunk_bytes,
                                                      report=report)
        if output_type == OutputType.SUBWORD:
            return self.bpe_cython.encode_file_subword(path, out, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, chunk_bytes=chunk_bytes,
                                                       report=report)
        return self.bpe_cython.encode_file(path, out=out, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, chunk_bytes=chunk_bytes,
                                           report=report)

    def encode_subword_tensor(self, sentences, bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0, device=None,
                              as_str: bool = False):
        """SUBWORD output made on the device: `sentences` as encode_tensor takes them -> (uint8 text tensor, int64 line_off [n + 1]) on the device,
        line i = text[line_off[i]:line_off[i + 1]] = every piece followed by a space, then a newline; as_str=True: the lines as list[str]"""
        from . import tensor
        return tensor.encode_subword_tensor(self, sentences, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, device=device, as_str=as_str)

    def encode_text_subword_tensor(self, text, bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0, as_str: bool = False):
        """the same for `text` as encode_text_tensor takes it, one sentence per line"""
        from . import tensor
        return tensor.encode_text_subword_tensor(self, text, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, as_str=as_str)

    # ---- where in the input every token came from (include/yttm_mi355x.h "Byte spans"; the reference has no counterpart)
    def encode_spans_tensor(self, sentences, bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0, padded: bool = True,
                            width: Optional[int] = None, pad_id: Optional[int] = None, device=None):
        """encode_tensor and, for every id, the bytes of its sentence it stands for: (ids [n, width], lengths [n], spans [n, width, 2]), or with
        padded=False (ids [n_ids], offsets [n + 1], spans [n_ids, 2]); ids, lengths and spans are int32, spans = (start, end) in bytes from the
        sentence's first byte, (0, 0) behind a row's last id.  A token without text of its own (<BOS>, <EOS>, a lone "▁") has an empty span."""
        from . import tensor
        return tensor.encode_spans_tensor(self, sentences, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, padded=padded, width=width,
                                          pad_id=pad_id, device=device)

    def encode_text_spans_tensor(self, text, bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0, padded: bool = True,
                                 width: Optional[int] = None, pad_id: Optional[int] = None):
        """the same for `text` as encode_text_tensor takes it, one sentence per line; the spans count from the line's first byte"""
        from . import tensor
        return tensor.encode_text_spans_tensor(self, text, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, padded=padded, width=width,
                                               pad_id=pad_id)

    def encode_with_spans(self, sentences: List[str], bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0,
                          unit: str = "char"):
        """-> (ids per sentence, (start, end) per id): with unit="char" offsets into the str, so that s[start:end] is the token's text (an unknown
        run's for unk_id, "" for <BOS>, <EOS> and a lone "▁"); with unit="byte" offsets into s.encode().  Needs no torch."""
        if unit not in ("char", "byte"):
            raise ValueError('unit must be "char" or "byte"')
        _check_dropout(dropout_prob)
        sentences = list(sentences)
        blob, offs = _pack(sentences)
        ids, off, spans = self.bpe_cython.encode_packed_spans(blob, offs, bos, eos, reverse, dropout_prob)
        spans = spans.astype(np.int64)
        if unit == "char" and len(blob) != sum(map(len, sentences)):
            # code points in front of a byte = the bytes in front of it that are no continuation bytes
            raw = np.frombuffer(blob, np.uint8)
            lead = np.zeros(len(raw) + 1, np.int64)
            np.cumsum((raw & 0xC0) != 0x80, out=lead[1:])
            base = np.repeat(offs[:-1].astype(np.int64), np.diff(off.astype(np.int64)))
            spans = lead[spans + base[:, None]] - lead[base][:, None]
        o, ids_l, sp_l = off.tolist(), ids.tolist(), spans.tolist()
        return ([ids_l[o[i]:o[i + 1]] for i in range(len(sentences))], [[tuple(p) for p in sp_l[o[i]:o[i + 1]]] for i in range(len(sentences))])

    # ---- how often every token is used (include/yttm_mi355x.h "Token frequencies"; the reference has no counterpart)
    def id_counts_tensor(self, ids=None, n_bins: Optional[int] = None, accumulate: bool = False):
        """Token frequencies made on the device -> an int64 tensor [n_bins + 1] on the encoder's device (the library's uint64 values viewed as int64,
        as the offsets tensors are): entry v the ids equal to v, the last entry the ids outside [0, n_bins).  n_bins=None: the vocabulary's size.
        ids=None counts the pending result of the last *_tensor encode or parse call, which stays pending; else `ids` is an int32 CUDA tensor of
        any shape, contiguous, counted flat (a padded matrix counts its pad values too).  accumulate=True adds to the counts of the calls before."""
        from . import tensor
        return tensor.id_counts_tensor(self, ids=ids, n_bins=n_bins, accumulate=accumulate)

    def count_file(self, path, bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0, chunk_bytes: Optional[int] = None,
                   report: bool = False):
        """A text file, one sentence per line -> np.uint64 counts [vocab_size + 1] of the ids encode_file gives for it, counted on the device piece by
        piece: only the counts come down.  The last entry counts ids outside the vocabulary (0 for an encode).  report=True: (counts, the call's
        report as a dict).  Needs no torch."""
        return self.bpe_cython.encode_file_counts(path, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, chunk_bytes=chunk_bytes, report=report)

    # ---- rows of exactly seq_len ids for language-model training (include/yttm_mi355x.h "Training blocks"; the reference has no counterpart)
    def encode_blocks_tensor(self, sentences, seq_len: int, mode: str = "stream", bos: bool = False, eos: bool = False, reverse: bool = False,
                             dropout_prob: float = 0, pad_id: Optional[int] = None, tail: str = "pad", device=None):
        """encode_tensor's sentences packed on the device into rows of exactly seq_len ids -> Blocks(rows, seg, pos, frags, row_frags), tensors on
        the encoder's device: rows, seg, pos int32 [n_rows, seq_len] (the ids; the 1-based number of the id's fragment within its row, 0 on padding;
        the id's index within its fragment), frags int32 [n_frags, 2] ((flat start, length) of every fragment), row_frags int64 [n_rows + 1].
        mode="stream" concatenates the sentences and cuts every seq_len ids; mode="whole" places sentences whole, several to a row (a sentence
        longer than seq_len raises).  tail: "pad" emits the incomplete last row with pad_id (default: the model's <PAD>) behind its ids, "keep" keeps
        it as this object's open row, which the next blocks call continues (blocks_flush_tensor ends it), "drop" discards it."""
        from . import tensor
        return tensor.encode_blocks_tensor(self, sentences, seq_len, mode=mode, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, pad_id=pad_id,
                                           tail=tail, device=device)

    def encode_text_blocks_tensor(self, text, seq_len: int, mode: str = "stream", bos: bool = False, eos: bool = False, reverse: bool = False,
                                  dropout_prob: float = 0, pad_id: Optional[int] = None, tail: str = "pad"):
        """the same for `text` as encode_text_tensor takes it, one sentence per line"""
        from . import tensor
        return tensor.encode_text_blocks_tensor(self, text, seq_len, mode=mode, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, pad_id=pad_id,
                                                tail=tail)

    def blocks_tensor(self, ids=None, lengths=None, offsets=None, seq_len: int = 0, mode: str = "stream", pad_id: Optional[int] = None, tail: str = "pad"):
        """packs ids this object did not encode: `ids`, `lengths`, `offsets` as decode_tensor takes them (a 2-D padded matrix with lengths, or 1-D
        int32 ids with offsets [n + 1]); ids=None packs the pending result of the last *_tensor encode or parse call -> Blocks as encode_blocks_tensor"""
        from . import tensor
        return tensor.blocks_tensor(self, ids=ids, lengths=lengths, offsets=offsets, seq_len=seq_len, mode=mode, pad_id=pad_id, tail=tail)

    def blocks_flush_tensor(self, pad_id: Optional[int] = None):
        """the open row as Blocks of 0 or 1 rows; the open row is empty afterwards"""
        from . import tensor
        return tensor.blocks_flush_tensor(self, pad_id=pad_id)

    def blocks_open(self):
        """(ids in the open row, its seq_len, its mode as "stream" / "whole"), or (0, 0, None) when it is empty"""
        f, L, mode = self.bpe_cython.blocks_open()
        return (f, L, "whole" if mode else "stream") if f else (0, 0, None)

    def blocks_discard(self):
        """empties the open row without emitting it"""
        self.bpe_cython.blocks_discard()

    def encode_file_blocks(self, path, out: str, seq_len: int, mode: str = "stream", bos: bool = False, eos: bool = False, reverse: bool = False,
                           dropout_prob: float = 0, pad_id: Optional[int] = None, drop_last: bool = False, chunk_bytes: Optional[int] = None,
                           report: bool = False):
        """A text file, one sentence per line -> OUT.rows (int32 [n_rows, seq_len]) and OUT.frags (uint64 [n_frags, 2], (flat start, length) over the
        whole file), packed on the device piece by piece; the files do not depend on chunk_bytes.  drop_last discards the incomplete last row
        instead of padding it.  Returns (n_rows, n_frags, n_lines, n_ids), or with report=True the call's report (a dict).  Needs no torch."""
        core = self.bpe_cython
        if mode not in core.MODES:
            raise ValueError('mode must be "stream" or "whole"')
        if pad_id is None:
            pad_id = self.subword_to_id("<PAD>")
            if not drop_last and (pad_id == -1 or self.id_to_subword(pad_id) != "<PAD>"):
                raise ValueError("the model was trained without <PAD> (pad_id=-1): pass pad_id")
        return core.encode_file_blocks(path, out, seq_len, core.MODES[mode], bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, pad_value=pad_id,
                                       tail=2 if drop_last else 0, chunk_bytes=chunk_bytes, report=report)

    # ---- sentences sorted by length and cut into batches under a token budget (include/yttm_mi355x.h "Batches by length"; the reference has no counterpart)
    def encode_batches_tensor(self, sentences, max_tokens: int, max_sentences: int = 0, min_len: int = 0, max_len: int = 0, left_pad: bool = False,
                              bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0, pad_id: Optional[int] = None, device=None):
        """encode_tensor's sentences sorted by length on the device and cut into batches of at most max_tokens padded ids (and max_sentences rows;
        0: no limit) -> Batches(order, batch_first, widths, batch_off, ids, n_kept), tensors on the encoder's device.  len(b) is the number of
        batches, b[k] = (sentence indices [rows], matrix [rows, width]): the matrix is a view of b.ids, its rows padded with pad_id (default: the
        model's <PAD>) on the right, with left_pad on the left.  Sentences shorter than min_len or longer than max_len (0: none) are left out; a
        kept sentence longer than max_tokens raises.  Two sides: plan with batches_plan_tensor(torch.maximum(len_src, len_tgt), ...) and
        gather each side with batches_gather_tensor."""
        from . import tensor
        return tensor.encode_batches_tensor(self, sentences, max_tokens, max_sentences=max_sentences, min_len=min_len, max_len=max_len, left_pad=left_pad, bos=bos,
                                            eos=eos, reverse=reverse, dropout_prob=dropout_prob, pad_id=pad_id, device=device)

    def encode_text_batches_tensor(self, text, max_tokens: int, max_sentences: int = 0, min_len: int = 0, max_len: int = 0, left_pad: bool = False,
                                   bos: bool = False, eos: bool = False, reverse: bool = False, dropout_prob: float = 0, pad_id: Optional[int] = None):
        """the same for `text` as encode_text_tensor takes it, one sentence per line"""
        from . import tensor
        return tensor.encode_text_batches_tensor(self, text, max_tokens, max_sentences=max_sentences, min_len=min_len, max_len=max_len, left_pad=left_pad, bos=bos,
                                                 eos=eos, reverse=reverse, dropout_prob=dropout_prob, pad_id=pad_id)

    def batches_plan_tensor(self, lengths, max_tokens: int, max_sentences: int = 0, min_len: int = 0, max_len: int = 0):
        """the plan alone from an int32 tensor of lengths on the encoder's device -> Batches whose widths, batch_off and ids are None"""
        from . import tensor
        return tensor.batches_plan_tensor(self, lengths, max_tokens, max_sentences=max_sentences, min_len=min_len, max_len=max_len)

    def batches_gather_tensor(self, ids, lengths=None, offsets=None, pad_id: Optional[int] = None, left_pad: bool = False):
        """the batches of the last plan for one side: `ids`, `lengths`, `offsets` as blocks_tensor takes them (a 2-D padded matrix with lengths, or
        1-D int32 ids with offsets [n + 1]) -> Batches"""
        from . import tensor
        return tensor.batches_gather_tensor(self, ids, lengths=lengths, offsets=offsets, pad_id=pad_id, left_pad=left_pad)

    # ---- encode with only the tokens a corpus uses often enough (include/yttm_mi355x.h "Encode under a restricted vocabulary")
    def set_vocabulary(self, allowed=None, counts=None, threshold: int = 1):
        """Restricts every later encode of this object to the allowed ids: a token outside them is split back into the two pieces it was merged
        from, and those again, down to allowed tokens or single chars (subword-nmt's --vocabulary / --vocabulary-threshold).  `allowed`: a bool
        mask [vocab_size]; or `counts`: what count_file / id_counts_tensor return (its last entry, the ids outside the vocabulary, is dropped),
        allowed = counts >= threshold.  Neither: the vocabulary is cleared.  Returns vocabulary_info()."""
        if allowed is not None and counts is not None:
            raise ValueError("pass allowed or counts, not both")
        if counts is not None:
            if hasattr(counts, "cpu"):
                counts = counts.cpu().numpy()
            counts = np.asarray(counts).ravel()
            V = self.vocab_size()
            if len(counts) not in (V, V + 1):
                raise ValueError("counts must have vocab_size or vocab_size + 1 entries, not %d" % len(counts))
            allowed = counts[:V].astype(np.uint64) >= int(threshold)
        elif allowed is not None:
            if hasattr(allowed, "cpu"):
                allowed = allowed.cpu().numpy()
            allowed = np.asarray(allowed).ravel()
        return self.bpe_cython.set_vocabulary(allowed)

    def vocabulary_info(self):
        """(allowed ids, ids that split, the longest expansion) of the vocabulary that is set; zeros when none is"""
        return self.bpe_cython.vocabulary_info()

    def vocabulary_stats(self):
        """(restricted calls, calls where nothing split, ids in, ids out) since this object was made"""
        return self.bpe_cython.vocabulary_stats()

    # ---- unknown characters as UTF-8 byte ids (include/yttm_mi355x.h "Byte fallback"; SentencePiece's byte_fallback)
    def set_byte_fallback(self, on: bool = True):
        """On: every encode of this object -- ids, tensors, SUBWORD text, id text, counts, blocks, batches, files -- gives the bytes of a run of
        characters outside the model's alphabet as the ids vocab_size() + b in place of the run's one <UNK>, so that decode(encode(s)) gives the
        text back; decode, id_to_subword ("<0xNN>"), subword_to_id and the counts know those 256 ids.  The model file and vocab_size() do not
        change.  Spans are not defined while it is on.  Off (the default): nothing changes."""
        self.bpe_cython.set_byte_fallback(on)

    def byte_fallback(self):
        """the first byte id (vocab_size()) while the byte fallback is on, else None"""
        return self.vocab_size() if self.bpe_cython.byte_fallback() else None

    def byte_fallback_stats(self):
        """(calls of the pass, calls whose write pass was skipped, ids in, ids out) since this object was made"""
        return self.bpe_cython.byte_fallback_stats()

    def byte_fallback_tensor(self, ids, text, lengths=None, offsets=None, reverse: bool = False, padded: Optional[bool] = None,
                             width: Optional[int] = None, pad_id: Optional[int] = None):
        """The pass alone, on ids this object did not encode and the text they were made from: ids as restrict_tensor takes them, text a list of
        str or a pair (uint8 bytes, offsets) on the device, one sentence per row of ids.  Every <UNK> that stands for an unknown run of its sentence
        becomes the run's byte ids; an <UNK> without a run stays.  Needs the setting on.  The result as restrict_tensor gives it."""
        from . import tensor
        return tensor.byte_fallback_tensor(self, ids, text, lengths=lengths, offsets=offsets, reverse=reverse, padded=padded, width=width, pad_id=pad_id)

    # ---- added tokens: literal strings that are one id each and never split (include/yttm_mi355x.h "Added tokens"; SentencePiece's
    # user_defined_symbols, Hugging Face's added tokens)
    def set_added_tokens(self, tokens=None):
        """tokens: up to 4096 different strings of 1 .. 255 bytes without white space or U+2581 -- language tags, separators, <mask>, sentinels,
        chat markers.  Token k is the id vocab_size() + 256 + k (behind the byte fallback's ids, whether that is on or not).  Every later encode of
        this object -- ids, tensors, id text, counts, blocks, batches, files -- matches them in the text (leftmost first, the longest at a
        position, never across a sentence's end) and gives each match as its one id; the text between the matches is encoded as sentences of
        its own.  decode, id_to_subword, subword_to_id and the counts know the ids.  The model file and vocab_size() do not change.  Spans are
        not defined while tokens are set, SUBWORD output only with the byte fallback on as well.  None (the default) clears the setting."""
        self.bpe_cython.set_added_tokens(tokens)

    def added_tokens(self):
        """a dict from token to id in the order of the ids, or None while nothing is set"""
        raw = self.bpe_cython.added_tokens_raw()
        first = self.vocab_size() + 256
        return {t.decode(): first + k for k, t in enumerate(raw)} if raw else None

    def added_tokens_stats(self):
        """(calls with the setting on, calls without a match, matches, sub-sentences encoded) since this object was made"""
        return self.bpe_cython.added_tokens_stats()

    def split_added_tensor(self, text, offsets=None):
        """The matcher alone: text a list of str, or a uint8 tensor on the device with int64 offsets [n + 1].  Returns three device tensors:
        sub_first int64 [n + 1] (the first sub-sentence of every sentence), sub_offsets int64 [n_sub + 1] (byte offsets into the text) and tok
        int32 [n_sub] (the token's index for a match, -1 for the text in front of, between and behind the matches).  Needs tokens set."""
        from . import tensor
        return tensor.split_added_tensor(self, text, offsets)

    def restrict_tensor(self, ids, lengths=None, offsets=None, reverse: bool = False, padded: Optional[bool] = None, width: Optional[int] = None,
                        pad_id: Optional[int] = None):
        """Restricts ids this object did not encode under the vocabulary that is set: `ids`, `lengths`, `offsets` as decode_tensor takes them (a
        2-D padded matrix with lengths, or 1-D ids with offsets [n + 1]) -> what encode_tensor returns; padded=None gives the input's form back."""
        from . import tensor
        return tensor.restrict_tensor(self, ids, lengths=lengths, offsets=offsets, reverse=reverse, padded=padded, width=width, pad_id=pad_id)

    # ---- decimal id text, one sentence per line: the format `yttm encode --output_type id` prints and `yttm decode` reads
    def decode_file(self, path, out: str, ignore_ids: Optional[Collection] = None, chunk_bytes: Optional[int] = None, report: bool = False):
        """A text file of decimal ids -> the text file `yttm decode < path` prints, written to `out`, made on the device file to file.  Returns
        (n_lines, n_ids, n_text_bytes), or with report=True the call's report (a dict).  Needs no torch."""
        return self.bpe_cython.decode_file(path, out, ignore_ids=ignore_ids, chunk_bytes=chunk_bytes, report=report)

    def decode_text_tensor(self, text, ignore_ids: Optional[Collection] = None, as_str: bool = True):
        """`text` as encode_text_tensor takes it, holding decimal ids, one sentence per line -> the decoded lines as list[str] (without their
        newlines), or with as_str=False (uint8 text, int64 line_off [n_lines + 1]) on the device, every line with its newline"""
        from . import tensor
        return tensor.decode_text_tensor(self, text, ignore_ids=ignore_ids, as_str=as_str)

    def parse_ids_tensor(self, text, padded: bool = False, width: Optional[int] = None, pad_id: Optional[int] = None):
        """`text` as encode_text_tensor takes it, holding decimal ids, one sentence per line -> the ids as encode_text_tensor returns them"""
        from . import tensor
        return tensor.parse_ids_tensor(self, text, padded=padded, width=width, pad_id=pad_id)

    def decode_tensor(self, ids, lengths=None, offsets=None, ignore_ids: Optional[Collection] = None, as_str: bool = True):
        from . import tensor
        return tensor.decode_tensor(self, ids, lengths=lengths, offsets=offsets, ignore_ids=ignore_ids, as_str=as_str)

    def __getstate__(self):
        return {"model": self.model, "n_threads": self.n_threads}

    def __setstate__(self, dict):
        self.model = dict["model"]
        self.n_threads = dict["n_threads"]
        self.bpe_cython = _Core(model_path=self.model, n_threads=self.n_threads)
