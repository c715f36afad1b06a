"""The read sequences of an assembly graph as ONE packed store (include/gnm.h, "contig sequences").

The reference keeps a Python string per NODE, so both strands of every read (graph_parser.py:252-254: node 2i is read i, node
2i + 1 its reverse complement).  Here one entry per READ holds the + strand; node v is read v >> 1 and an odd v is formed on
the fly.  Four bits per base in the BAM nibble code "=ACMGRSVTWYHKDBN": A=1, C=2, G=4, T=8, an IUPAC ambiguity code is the OR
of its bases, N=15 -- so the complement of a code is its four bits in reverse order, for every code, and the reverse strand needs
no table.  Two bases per byte, low nibble first.  Read r starts at nibble base_off[r], a multiple of 32 (a 16-byte boundary);
pad nibbles are 0.

Packing is host numpy through a 256-entry table, once per data set; `decode.contig_sequences` reads the store on the device."""
from __future__ import annotations

import gzip
from typing import Iterable, Iterator, List, Optional, Tuple

import numpy as np
import torch

__all__ = ["ReadStore", "LETTERS", "complement_code", "read_records"]

LETTERS = "=ACMGRSVTWYHKDBN"
_ALIGN = 32                                       # nibbles: every read starts on a 16-byte boundary

_ENCODE = np.zeros(256, np.uint8)                 # 0: not a base
for _c, _ch in enumerate(LETTERS):
    if _c:
        _ENCODE[ord(_ch)] = _ENCODE[ord(_ch.lower())] = _c
_ENCODE[ord("U")] = _ENCODE[ord("u")] = 8         # RNA: U reads as T
_DECODE = np.frombuffer(LETTERS.encode(), np.uint8)
_BREV4 = np.array([int(f"{c:04b}"[::-1], 2) for c in range(16)], np.uint8)


def complement_code(code):
    """The code of the complement: the four bits reversed (an involution; A<->T, C<->G, N, S and W stay)."""
    return _BREV4[np.asarray(code, np.int64)]


def _open(path):
    path = str(path)
    with open(path, "rb") as fh:
        magic = fh.read(2)
    return gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")


def read_records(path) -> Iterator[Tuple[str, bytes]]:
    """(name, sequence) of every record of a FASTA or FASTQ file, plain or gzip (by its magic bytes).  Sequence lines of a record
    are joined; a FASTQ record's quality is as long as its sequence and is skipped.  The sequence is NOT checked here."""
    with _open(path) as fh:
        line = fh.readline()
        while line and not line.strip():
            line = fh.readline()
        while line:
            head = line.rstrip(b"\r\n")
            if head[:1] not in (b">", b"@"):
                raise ValueError(f"{path}: expected a '>' or '@' header, found {head[:40]!r}")
            name = head[1:].decode(errors="replace")
            fastq = head[:1] == b"@"
            parts: List[bytes] = []
            line = fh.readline()
            while line and line[:1] != (b"+" if fastq else b">"):
                parts.append(line.rstrip(b"\r\n"))
                line = fh.readline()
            seq = b"".join(parts)
            if fastq:
                if not line:
                    raise ValueError(f"{path}: record {name.split()[0] if name else ''!r} has no '+' line")
                got = 0
                line = fh.readline()
                while line and got < len(seq):
                    got += len(line.rstrip(b"\r\n"))
                    line = fh.readline()
                if got != len(seq):
                    raise ValueError(f"{path}: record {name!r}: {len(seq)} bases, {got} quality values")
            while line and not line.strip():
                line = fh.readline()
            yield name, seq


class ReadStore:
    """packed uint8 [bytes] (whole 16-byte groups), base_off int64 [R] (nibble index of read r's first base, a multiple of 32),
    length int64 [R]; all three torch tensors on one device.  `names`: the records' names when read from a file, else None."""

    def __init__(self, packed, base_off, length, names: Optional[List[str]] = None):
        as_t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dt).contiguous()  # noqa: E731
        self.packed, self.base_off, self.length = as_t(packed, torch.uint8), as_t(base_off, torch.int64), as_t(length, torch.int64)
        self.names = list(names) if names is not None else None
        if self.base_off.numel() != self.length.numel() or (self.names is not None and len(self.names) != self.length.numel()):
            raise ValueError("ReadStore: base_off, length and names need one entry per read")
        if not (self.packed.device == self.base_off.device == self.length.device):
            raise ValueError("ReadStore: packed, base_off and length must live on one device")

    def __len__(self):
        return int(self.length.numel())

    @property
    def device(self):
        return self.packed.device

    # ---- building -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_sequences(cls, seqs: Iterable, names: Optional[List[str]] = None) -> "ReadStore":
        """Pack str / bytes sequences.  Lower case folds to upper, U reads as T; any other character -- '-', '*', '=', a digit,
        white space inside a sequence -- raises ValueError naming the read and the position."""
        codes, lengths = [], []
        for r, s in enumerate(seqs):
            raw = s.encode("latin-1", errors="replace") if isinstance(s, str) else bytes(s)
            c = _ENCODE[np.frombuffer(raw, np.uint8)]
            bad = np.flatnonzero(c == 0)
            if bad.size:
                who = f"read {r}" + (f" ({names[r]!r})" if names is not None and r < len(names) else "")
                raise ValueError(f"{who}: character {chr(raw[bad[0]])!r} at position {int(bad[0])} is not a base "
                                 f"(A C G T U, the IUPAC ambiguity letters and N are)")
            codes.append(c)
            lengths.append(c.size)
        length = np.asarray(lengths, np.int64).reshape(-1)
        span = (length + _ALIGN - 1) // _ALIGN * _ALIGN
        base_off = np.concatenate([[0], np.cumsum(span)[:-1]]).astype(np.int64) if length.size else np.zeros(0, np.int64)
        nib = np.zeros(int(span.sum()), np.uint8)
        for c, o in zip(codes, base_off):
            nib[o:o + c.size] = c
        packed = nib[0::2] | (nib[1::2] << 4)
        return cls(packed, base_off, length, names)

    @classmethod
    def from_fasta(cls, path) -> "ReadStore":
        """The records of a FASTA or FASTQ file (plain or .gz), in file order: record i is read i, nodes 2i and 2i + 1."""
        names, seqs = [], []
        for name, seq in read_records(path):
            names.append(name)
            seqs.append(seq)
        return cls.from_sequences(seqs, names)

    # ---- the host route ---------------------------------------------------------------------------------------------------------
    def codes(self, node: int) -> np.ndarray:
        """uint8 [length]: the 4-bit codes of node's strand, first base first."""
        r = int(node) >> 1
        if not 0 <= r < len(self):
            raise IndexError(f"node {node}: the store holds {len(self)} reads")
        o, n = int(self.base_off[r]), int(self.length[r])
        if o < 0 or n < 0 or o % 2 or o + n > 2 * self.packed.numel():
            raise ValueError(f"read {r}: nibbles [{o}, {o + n}) do not lie inside the store")
        b = self.packed[o // 2:(o + n + 1) // 2].cpu().numpy()
        c = np.empty(2 * b.size, np.uint8)
        c[0::2], c[1::2] = b & 15, b >> 4
        c = c[:n]
        return _BREV4[c[::-1]] if int(node) & 1 else c

    def sequence(self, node: int) -> str:
        """The sequence of NODE `node` as the reference's reads[node]: read node >> 1, reverse-complemented when node is odd."""
        return _DECODE[self.codes(node)].tobytes().decode()

    # ---- housekeeping -----------------------------------------------------------------------------------------------------------
    def validate(self) -> "ReadStore":
        """One host check that every read lies inside `packed` and starts on a 16-byte boundary."""
        off, n = self.base_off.cpu().numpy(), self.length.cpu().numpy()
        if self.packed.numel() % 16:
            raise ValueError(f"ReadStore: packed holds {self.packed.numel()} bytes, not whole 16-byte groups")
        bad = np.flatnonzero((off < 0) | (n < 0) | (off % _ALIGN != 0) | (off + n > 2 * self.packed.numel()))
        if bad.size:
            r = int(bad[0])
            raise ValueError(f"ReadStore: read {r} (base_off {int(off[r])}, length {int(n[r])}) is misaligned or outside the "
                             f"{2 * self.packed.numel()} nibbles of the store")
        return self

    def to(self, device) -> "ReadStore":
        return ReadStore(self.packed.to(device), self.base_off.to(device), self.length.to(device), self.names)

    def save(self, path) -> None:
        """One .npz: packed, base_off, length and, when there are any, names."""
        arrs = {"packed": self.packed.cpu().numpy(), "base_off": self.base_off.cpu().numpy(), "length": self.length.cpu().numpy()}
        if self.names is not None:
            arrs["names"] = np.asarray(self.names, dtype=np.str_)
        with open(path, "wb") as fh:
            np.savez(fh, **arrs)

    @classmethod
    def load(cls, path) -> "ReadStore":
        with np.load(path, allow_pickle=False) as z:
            names = z["names"].tolist() if "names" in z.files else None
            return cls(z["packed"], z["base_off"], z["length"], names).validate()
