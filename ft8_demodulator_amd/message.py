"""The message layer of the FT8 protocol: 77-bit payload <-> text, callsign hashes.

unpack77 / hash_call call the library's host entry points (ft8_unpack77_host, ft8_hash_call: the
same csrc/msg77.h the device kernel k_unpack77 runs) and need no GPU.  pack77 is written here in
Python, independently of msg77.h, so a round trip through both checks one against the other.

No reference counterpart: the reference stops at the payload (build-defined, like FT8_FLAG_TOPK).

Message types: standard (i3 = 1, 2), one non-standard callsign (i3 = 4), free text (i3 = 0,
n3 = 0), telemetry (i3 = 0, n3 = 5).  DESIGN.md has the field layouts.
"""
from __future__ import annotations

import ctypes
import re

import numpy as np

from . import _lib
from ._lib import TEXT_DTYPE  # noqa: F401  (public here)

NTOKENS = 2063592
MAX22 = 4194304
MAXGRID4 = 32400

A1 = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
A2 = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
A3 = "0123456789"
A4 = " ABCDEFGHIJKLMNOPQRSTUVWXYZ"
A38 = A1 + "/"
A42 = A1 + "+-./?"

ST_OK, ST_UNDECODED, ST_RANGE, ST_NOT_OK = 0, 1, 2, 3


# ---- library side ---------------------------------------------------------------------------------
def unpack77(payloads) -> np.ndarray:
    """10-byte payload(s) -> ft8_text record(s) (TEXT_DTYPE), on the host.

    bytes / bytearray / a [10] array give one record (a 0-d structured scalar), an [n, 10] array or
    a list of payloads gives an array of n records.  dup_of is -1 throughout."""
    raw = (bytes, bytearray, memoryview)
    single = isinstance(payloads, raw)
    if isinstance(payloads, (list, tuple)):
        payloads = [np.frombuffer(bytes(p), dtype=np.uint8) if isinstance(p, raw) else p for p in payloads]
        if not payloads:
            payloads = np.zeros((0, 10), dtype=np.uint8)
    a = np.frombuffer(bytes(payloads), dtype=np.uint8) if single else np.asarray(payloads, dtype=np.uint8)
    if single or a.ndim == 1:
        single = True
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] != 10:
        raise ValueError("a payload is 10 bytes")
    a = np.ascontiguousarray(a)
    out = np.zeros(a.shape[0], dtype=TEXT_DTYPE)
    rc = _lib.lib().ft8_unpack77_host(a.ctypes.data_as(ctypes.c_void_p), int(a.shape[0]),
                                      out.ctypes.data_as(ctypes.c_void_p))
    if rc != _lib.FT8_OK:
        raise ValueError(f"ft8_unpack77_host failed with code {rc}")
    return out[0] if single else out


def hash_call(call: str) -> int:
    """n22 of a callsign (n12 = n22 >> 10, n10 = n22 >> 12).  ValueError for a character outside
    " 0-9A-Z/" or more than 11 characters."""
    v = ctypes.c_uint32()
    try:
        raw = call.encode("ascii")
    except UnicodeEncodeError:
        raise ValueError(f"not a callsign: {call!r}") from None
    if _lib.lib().ft8_hash_call(raw, ctypes.byref(v)) != _lib.FT8_OK:
        raise ValueError(f"not a callsign: {call!r}")
    return int(v.value)


def text_of(record) -> str:
    return bytes(record["text"]).split(b"\0", 1)[0].decode("ascii")


# ---- pack77 (pure Python) -------------------------------------------------------------------------
def _hash22_py(call: str) -> int:
    m = 0
    for ch in call.ljust(11):
        m = m * 38 + A38.index(ch)
    return ((47055833459 * m) & 0xFFFFFFFFFFFFFFFF) >> 42


def _check_call38(call: str) -> str:
    if not (1 <= len(call) <= 11) or any(ch not in A38 or ch == " " for ch in call):
        raise ValueError(f"not a callsign: {call!r}")
    return call


def _pack_std_call(c: str) -> int:
    """A standard callsign as it is rendered -> its value n (n28 = NTOKENS + MAX22 + n)."""
    if c.startswith("3DA0") and 4 < len(c) <= 7:
        c = "3D0" + c[4:]
    elif len(c) >= 3 and c.startswith("3X") and c[2].isalpha():
        c = "Q" + c[2:]
    elif (c.startswith("3D0") and len(c) > 3) or (len(c) >= 2 and c[0] == "Q" and c[1].isalpha()):
        raise ValueError(f"{c!r} is rendered in another spelling")  # 3DA0..., 3X...
    for c6 in (c, " " + c):
        if len(c6) > 6 or len(c6) < 3:
            continue
        c6 = c6.ljust(6)
        if (c6[0] in A1 and c6[1] in A2 and c6[2] in A3 and all(ch in A4 for ch in c6[3:])
                and c6.strip() == c and " " not in c):
            n = A1.index(c6[0])
            n = n * 36 + A2.index(c6[1])
            n = n * 10 + A3.index(c6[2])
            for ch in c6[3:]:
                n = n * 27 + A4.index(ch)
            return n
    raise ValueError(f"not a standard callsign: {c!r}")


_RE_UPPER = re.compile(r"[A-Z]{1,4}\Z")
_RE_NNN = re.compile(r"[0-9]{3}\Z")
_RE_REPORT = re.compile(r"(R?)([+-])([0-9]{2})\Z")
_RE_GRID = re.compile(r"[A-R]{2}[0-9]{2}\Z")
_WORDS = {"RRR": 2, "RR73": 3, "73": 4}


def _std_calls(tok, i):
    """Every reading of tok[i:] as one call of a standard message: (n28, suffix, next index)."""
    if i >= len(tok):
        return
    t = tok[i]
    if t == "DE":
        yield 0, "", i + 1
    elif t == "QRZ":
        yield 1, "", i + 1
    elif t == "CQ":
        if i + 1 < len(tok) and _RE_NNN.match(tok[i + 1]):
            yield 3 + int(tok[i + 1]), "", i + 2
        if i + 1 < len(tok) and _RE_UPPER.match(tok[i + 1]):
            n = 0
            for ch in tok[i + 1].rjust(4):
                n = n * 27 + A4.index(ch)
            yield 1003 + n, "", i + 2
        yield 2, "", i + 1
    else:
        sfx = ""
        if t.endswith("/R") or t.endswith("/P"):
            t, sfx = t[:-2], t[-1]
        try:
            if t.startswith("<") and t.endswith(">"):
                yield NTOKENS + _hash22_py(_check_call38(t[1:-1])), sfx, i + 1  # "<...>" raises
            else:
                yield NTOKENS + MAX22 + _pack_std_call(t), sfx, i + 1
        except ValueError:
            return


def _std_extra(tok):
    """The tokens after the two calls -> (ir, g15), or None."""
    if not tok:
        return 0, MAXGRID4 + 1
    if len(tok) == 1:
        t = tok[0]
        if t in _WORDS:
            return 0, MAXGRID4 + _WORDS[t]
        m = _RE_REPORT.match(t)
        if m:
            snr = int(m.group(3)) * (-1 if m.group(2) == "-" else 1)
            if abs(snr) > 50 or (snr == 0 and m.group(2) == "-"):
                return None
            irpt = snr + 35 + (101 if snr < -30 else 0)
            return int(bool(m.group(1))), MAXGRID4 + irpt
        if _RE_GRID.match(t):
            return 0, _grid(t)
        return None
    if len(tok) == 2 and tok[0] == "R" and _RE_GRID.match(tok[1]):
        return 1, _grid(tok[1])
    return None


def _grid(g: str) -> int:
    return ((ord(g[0]) - 65) * 18 + (ord(g[1]) - 65)) * 100 + (ord(g[2]) - 48) * 10 + (ord(g[3]) - 48)


def _pack_std(tok):
    for n28a, sa, i in _std_calls(tok, 0):
        for n28b, sb, j in _std_calls(tok, i):
            extra = _std_extra(tok[j:])
            if extra is None:
                continue
            sfx = {sa, sb} - {""}
            if len(sfx) > 1:
                continue
            i3 = 2 if sfx == {"P"} else 1
            ir, g15 = extra
            v = n28a
            v = (v << 1) | int(bool(sa))
            v = (v << 28) | n28b
            v = (v << 1) | int(bool(sb))
            v = (v << 1) | ir
            v = (v << 15) | g15
            return (v << 3) | i3
    return None


def _pack_nonstd(tok):
    def c58(call):
        n = 0
        for ch in _check_call38(call).rjust(11):
            n = n * 38 + A38.index(ch)
        return n

    def hashed(t):
        if len(t) > 2 and t.startswith("<") and t.endswith(">") and t != "<...>":
            return _hash22_py(_check_call38(t[1:-1])) >> 10
        return None

    try:
        if len(tok) == 2 and tok[0] == "CQ":
            h12, n58, iflip, nrpt, icq = _hash22_py(_check_call38(tok[1])) >> 10, c58(tok[1]), 0, 0, 1
        elif len(tok) in (2, 3):
            nrpt = 0
            if len(tok) == 3:
                if tok[2] not in _WORDS:
                    return None
                nrpt = _WORDS[tok[2]] - 1
            icq = 0
            if hashed(tok[0]) is not None and hashed(tok[1]) is None:
                h12, n58, iflip = hashed(tok[0]), c58(tok[1]), 0
            elif hashed(tok[1]) is not None and hashed(tok[0]) is None:
                h12, n58, iflip = hashed(tok[1]), c58(tok[0]), 1
            else:
                return None
        else:
            return None
    except ValueError:
        return None
    v = h12
    v = (v << 58) | n58
    v = (v << 1) | iflip
    v = (v << 2) | nrpt
    v = (v << 1) | icq
    return (v << 3) | 4


def _bytes77(v: int) -> bytes:
    return (v << 3).to_bytes(10, "big")


def pack_telemetry(hexstr: str) -> bytes:
    """Up to 18 hex digits (71 bits) -> a telemetry payload (i3 = 0, n3 = 5)."""
    if not (1 <= len(hexstr) <= 18) or any(ch not in "0123456789abcdefABCDEF" for ch in hexstr):
        raise ValueError(f"telemetry is 1..18 hex digits, got {hexstr!r}")
    f71 = int(hexstr, 16)
    if f71 >> 71:
        raise ValueError("telemetry holds 71 bits")
    return _bytes77((f71 << 6) | (5 << 3))


def pack77(text: str) -> bytes:
    """Message text as unpack77 renders it -> the 10-byte payload.  A hashed callsign is written
    <CALL> (its hash is packed).  ValueError for anything the unpacker cannot render."""
    if not isinstance(text, str):
        raise ValueError("text must be a str")
    tok = text.split(" ")
    if all(tok):  # single spaces only, no leading / trailing space
        v = _pack_std(tok)
        if v is None:
            v = _pack_nonstd(tok)
        if v is not None:
            return _bytes77(v)
    if len(text) == 18 and all(ch in "0123456789ABCDEF" for ch in text) and text[0] in "01234567":
        return pack_telemetry(text)
    if len(text) <= 13 and all(ch in A42 for ch in text) and text == text.strip(" "):
        f71 = 0
        for ch in text.rjust(13):
            f71 = f71 * 42 + A42.index(ch)
        return _bytes77(f71 << 6)
    raise ValueError(f"cannot pack {text!r} as an FT8 message")


# ---- callsign hash table --------------------------------------------------------------------------
class CallsignTable:
    """What a receiver remembers to resolve hashed callsigns: n22, n12 and n10 -> call, the most
    recently learned call winning."""

    def __init__(self):
        self._by = {22: {}, 12: {}, 10: {}}

    def add(self, call: str, n22: int = None) -> None:
        n22 = hash_call(call) if n22 is None else int(n22)
        self._by[22][n22] = call
        self._by[12][n22 >> 10] = call
        self._by[10][n22 >> 12] = call

    def learn(self, records) -> None:
        """Take learn_call / learn_hash22 of text records (a TEXT_DTYPE array or one record)."""
        for r in np.atleast_1d(records):
            call = bytes(r["learn_call"]).split(b"\0", 1)[0].decode("ascii")
            if call and int(r["status"]) == ST_OK:
                self.add(call, int(r["learn_hash22"]))

    def lookup(self, value: int, bits: int):
        return self._by.get(int(bits), {}).get(int(value))

    def resolve(self, record) -> str:
        """The record's text with <CALL> for every <...> whose hash is known."""
        parts = text_of(record).split("<...>")
        out = parts[0]
        for k, rest in enumerate(parts[1:]):
            call = self.lookup(record["hash"][k], record["hash_bits"][k]) if k < 2 else None
            out += ("<" + call + ">" if call else "<...>") + rest
        return out
