"""A small HDF5 subset in pure Python: enough to read what h5py writes with its default settings
(and therefore what Keras 3 writes into `model.weights.h5`), and to write files libhdf5 reads back.

Reader: superblock versions 0-3; object headers v1 and v2 (`OHDR`, with continuation blocks);
old-style groups (symbol-table message, v1 group B-tree of any depth, local heap, `SNOD` nodes)
and compact groups (link messages); dataspaces v1/v2 (scalar or simple); little- and big-endian
IEEE f16/f32/f64 and 8/16/32/64-bit integers; data layout v3 (compact, contiguous, chunked
without filters).  Unknown header messages and attributes are skipped.  Dense (fractal-heap)
groups, filtered chunks and anything else outside the subset raise `ValueError`, as does a
damaged or truncated file: every read is bounds-checked and every pointer walk remembers where
it has been, so a bad file ends in a `ValueError` naming the offset, never an `IndexError` or a
loop.

Writer: superblock v0, v1 object headers, symbol-table groups and contiguous datasets.  The
superblock's "group leaf node K" is sized so that every group fits in one `SNOD`, so each group
has a one-leaf B-tree (valid per the format specification; libhdf5 takes K from the superblock).
`SNOD` entries are sorted by name bytes, which libhdf5's binary search relies on.

API: `read(src) -> {"a/b/c": ndarray}`, `walk(src)` (os.walk-like over groups), and
`write(dst, tree)` with `tree` a nested dict of groups (dicts) and arrays.
"""
from __future__ import annotations

import io
import math
import struct
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Tuple, Union

import numpy as np

SIGNATURE = b"\x89HDF\r\n\x1a\n"

# header message types
_NIL, _DATASPACE, _LINK_INFO, _DATATYPE, _FILL_OLD, _FILL, _LINK = 0x0, 0x1, 0x2, 0x3, 0x4, 0x5, 0x6
_LAYOUT, _FILTERS, _CONT, _STAB = 0x8, 0xB, 0x10, 0x11

_MAX_DEPTH = 256            # group nesting / B-tree levels accepted before a file is called circular
_MAX_RANK = 32              # H5S_MAX_RANK


class _Buf:
    """Bounds-checked little-endian access to the file image."""

    def __init__(self, data: bytes) -> None:
        self.b = bytes(data)
        self.n = len(self.b)

    def need(self, off: int, size: int, what: str) -> None:
        if off < 0 or size < 0 or off + size > self.n:
            raise ValueError(f"hdf5: {what} at offset {off:#x} (+{size}) lies outside the "
                             f"{self.n}-byte file (truncated or damaged)")

    def u(self, off: int, size: int, what: str) -> int:
        self.need(off, size, what)
        return int.from_bytes(self.b[off:off + size], "little")

    def raw(self, off: int, size: int, what: str) -> bytes:
        self.need(off, size, what)
        return self.b[off:off + size]


class _Obj:
    __slots__ = ("addr", "msgs")

    def __init__(self, addr: int, msgs: List[Tuple[int, int, int, int]]) -> None:
        self.addr = addr
        self.msgs = msgs          # (type, flags, data offset, data size)

    def find(self, mtype: int) -> List[Tuple[int, int, int, int]]:
        return [m for m in self.msgs if m[0] == mtype]


class _Reader:
    def __init__(self, data: bytes) -> None:
        self.f = _Buf(data)
        self._objs: Dict[int, _Obj] = {}
        self._superblock()

    # ------------------------------------------------------------------ basics
    def addr(self, off: int, what: str) -> Optional[int]:
        """An address field: None for the undefined address, else the absolute file offset."""
        v = self.f.u(off, self.O, what)
        if v == (1 << (8 * self.O)) - 1:
            return None
        a = self.base + v
        if a >= self.f.n:
            raise ValueError(f"hdf5: {what} at offset {off:#x} points to {a:#x}, past the end of "
                             f"the {self.f.n}-byte file")
        return a

    def _superblock(self) -> None:
        f = self.f
        at = 0
        while True:
            if f.n >= at + 8 and f.b[at:at + 8] == SIGNATURE:
                break
            at = 512 if at == 0 else at * 2
            if at + 8 > f.n:
                raise ValueError("hdf5: no HDF5 signature at offset 0 or any power of two >= 512")
        ver = f.u(at + 8, 1, "superblock version")
        if ver in (0, 1):
            self.O = f.u(at + 13, 1, "size of offsets")
            self.L = f.u(at + 14, 1, "size of lengths")
            self._check_sizes(at)
            p = at + 24 + (4 if ver == 1 else 0)
            self.base = 0
            base = f.u(p, self.O, "base address")
            self.base = base
            entry = p + 4 * self.O
            self.root = self.addr(entry + self.O, "root group object header address")
        elif ver in (2, 3):
            self.O = f.u(at + 9, 1, "size of offsets")
            self.L = f.u(at + 10, 1, "size of lengths")
            self._check_sizes(at)
            p = at + 12
            self.base = 0
            self.base = f.u(p, self.O, "base address")
            self.root = self.addr(p + 3 * self.O, "root group object header address")
        else:
            raise ValueError(f"hdf5: superblock version {ver} at offset {at + 8:#x} is not supported "
                             "(0-3 are)")
        if self.root is None:
            raise ValueError(f"hdf5: superblock at offset {at:#x} has an undefined root group address")

    def _check_sizes(self, at: int) -> None:
        if self.O not in (2, 4, 8) or self.L not in (2, 4, 8):
            raise ValueError(f"hdf5: superblock at offset {at:#x}: size of offsets {self.O} / lengths "
                             f"{self.L} (2, 4 or 8 expected)")

    # ---------------------------------------------------------- object headers
    def obj(self, addr: int) -> _Obj:
        o = self._objs.get(addr)
        if o is None:
            if self.f.raw(addr, 4, "object header") == b"OHDR":
                o = _Obj(addr, self._ohdr_v2(addr))
            else:
                o = _Obj(addr, self._ohdr_v1(addr))
            self._objs[addr] = o
        return o

    def _ohdr_v1(self, addr: int) -> List[Tuple[int, int, int, int]]:
        f = self.f
        ver = f.u(addr, 1, "object header version")
        if ver != 1:
            raise ValueError(f"hdf5: object header at offset {addr:#x}: version {ver} (1, or an OHDR "
                             "signature, expected)")
        size = f.u(addr + 8, 4, "object header size")
        blocks = [(addr + 16, size)]
        msgs: List[Tuple[int, int, int, int]] = []
        seen = {addr + 16}
        while blocks:
            start, size = blocks.pop(0)
            f.need(start, size, "object header block")
            p, end = start, start + size
            while p + 8 <= end:
                mtype = f.u(p, 2, "message type")
                msize = f.u(p + 2, 2, "message size")
                mflags = f.u(p + 4, 1, "message flags")
                if p + 8 + msize > end:
                    raise ValueError(f"hdf5: message at offset {p:#x} (type {mtype:#x}, {msize} bytes) "
                                     f"overruns its object header block ending at {end:#x}")
                if mtype == _CONT:
                    blocks.append(self._continuation(p + 8, seen))
                else:
                    msgs.append((mtype, mflags, p + 8, msize))
                p += 8 + msize
        return msgs

    def _continuation(self, p: int, seen: set) -> Tuple[int, int]:
        a = self.addr(p, "continuation address")
        n = self.f.u(p + self.O, self.L, "continuation length")
        if a is None or a in seen:
            raise ValueError(f"hdf5: continuation message at offset {p:#x} points to "
                             f"{'nothing' if a is None else hex(a)} (undefined or already read)")
        seen.add(a)
        return a, n

    def _ohdr_v2(self, addr: int) -> List[Tuple[int, int, int, int]]:
        f = self.f
        ver = f.u(addr + 4, 1, "OHDR version")
        if ver != 2:
            raise ValueError(f"hdf5: OHDR at offset {addr:#x}: version {ver} (2 expected)")
        flags = f.u(addr + 5, 1, "OHDR flags")
        p = addr + 6
        if flags & 0x20:
            p += 16
        if flags & 0x10:
            p += 4
        w = 1 << (flags & 3)
        size = f.u(p, w, "OHDR chunk size")
        p += w
        crt = 2 if flags & 0x04 else 0
        blocks = [(p, size)]
        msgs: List[Tuple[int, int, int, int]] = []
        seen = {addr}
        first = True
        while blocks:
            start, size = blocks.pop(0)
            if not first:
                if f.raw(start, 4, "continuation block") != b"OCHK":
                    raise ValueError(f"hdf5: continuation block at offset {start:#x} lacks its OCHK "
                                     "signature")
                start, size = start + 4, size - 8      # signature ... checksum
            else:
                first = False
            f.need(start, size + 4, "OHDR chunk")
            q, end = start, start + size
            while q + 4 + crt <= end:
                mtype = f.u(q, 1, "message type")
                msize = f.u(q + 1, 2, "message size")
                mflags = f.u(q + 3, 1, "message flags")
                data = q + 4 + crt
                if data + msize > end:
                    raise ValueError(f"hdf5: message at offset {q:#x} (type {mtype:#x}, {msize} bytes) "
                                     f"overruns its OHDR chunk ending at {end:#x}")
                if mtype == _CONT:
                    blocks.append(self._continuation(data, seen))
                else:
                    msgs.append((mtype, mflags, data, msize))
                q = data + msize
        return msgs

    # ------------------------------------------------------------------ groups
    def is_group(self, o: _Obj) -> bool:
        return bool(o.find(_STAB) or o.find(_LINK) or o.find(_LINK_INFO))

    def is_dataset(self, o: _Obj) -> bool:
        return bool(o.find(_LAYOUT))

    def members(self, o: _Obj) -> List[Tuple[str, int]]:
        out: Dict[bytes, int] = {}
        for _t, _fl, p, _n in o.find(_LINK_INFO):
            heap = self.addr(p + 2 + (8 if self.f.u(p + 1, 1, "link info flags") & 1 else 0),
                             "link info fractal heap address")
            if heap is not None:
                raise ValueError(f"hdf5: group at offset {o.addr:#x} stores its links densely (fractal "
                                 f"heap at {heap:#x}): not supported")
        for _t, _fl, p, n in o.find(_STAB):
            btree = self.addr(p, "symbol table B-tree address")
            heap = self.addr(p + self.O, "symbol table local heap address")
            if btree is None or heap is None:
                raise ValueError(f"hdf5: symbol table message at offset {p:#x} has an undefined address")
            names = self._local_heap(heap)
            self._group_btree(btree, names, out, set(), None)
        for _t, _fl, p, n in o.find(_LINK):
            name, target = self._link(p, n)
            if target is not None:
                out[name] = target
        return sorted(((k.decode("utf-8", "replace"), v) for k, v in out.items()), key=lambda kv: kv[0].encode())

    def _local_heap(self, addr: int) -> Tuple[int, int]:
        f = self.f
        if f.raw(addr, 4, "local heap") != b"HEAP":
            raise ValueError(f"hdf5: local heap at offset {addr:#x} lacks its HEAP signature")
        size = f.u(addr + 8, self.L, "local heap data size")
        data = self.addr(addr + 8 + 2 * self.L, "local heap data address")
        if data is None:
            raise ValueError(f"hdf5: local heap at offset {addr:#x} has no data segment")
        f.need(data, size, "local heap data segment")
        return data, size

    def _heap_name(self, heap: Tuple[int, int], off: int, where: int) -> bytes:
        data, size = heap
        if off >= size:
            raise ValueError(f"hdf5: name offset {off} (at {where:#x}) is past the local heap's "
                             f"{size}-byte data segment")
        seg = self.f.b[data + off:data + size]
        end = seg.find(b"\0")
        if end < 0:
            raise ValueError(f"hdf5: name at heap offset {off} (at {where:#x}) is not NUL-terminated")
        return seg[:end]

    def _group_btree(self, addr: int, heap, out: Dict[bytes, int], seen: set, level: Optional[int]) -> None:
        f = self.f
        if addr in seen:
            raise ValueError(f"hdf5: group B-tree node at offset {addr:#x} is reached twice (cycle)")
        seen.add(addr)
        if f.raw(addr, 4, "group B-tree node") != b"TREE":
            raise ValueError(f"hdf5: group B-tree node at offset {addr:#x} lacks its TREE signature")
        ntype = f.u(addr + 4, 1, "B-tree node type")
        lvl = f.u(addr + 5, 1, "B-tree node level")
        used = f.u(addr + 6, 2, "B-tree entries used")
        if ntype != 0:
            raise ValueError(f"hdf5: B-tree node at offset {addr:#x} has type {ntype} in a group tree")
        if (level is not None and lvl != level) or lvl > _MAX_DEPTH:
            raise ValueError(f"hdf5: group B-tree node at offset {addr:#x} has level {lvl} "
                             f"({'any' if level is None else level} expected)")
        p = addr + 8 + 2 * self.O + self.L          # header, siblings, key 0
        f.need(p, used * (self.O + self.L), "B-tree entries")
        for i in range(used):
            child = self.addr(p + i * (self.O + self.L), "B-tree child address")
            if child is None:
                raise ValueError(f"hdf5: group B-tree node at offset {addr:#x}: child {i} is undefined")
            if lvl > 0:
                self._group_btree(child, heap, out, seen, lvl - 1)
            else:
                self._snod(child, heap, out, seen)

    def _snod(self, addr: int, heap, out: Dict[bytes, int], seen: set) -> None:
        f = self.f
        if addr in seen:
            raise ValueError(f"hdf5: symbol node at offset {addr:#x} is reached twice (cycle)")
        seen.add(addr)
        if f.raw(addr, 4, "symbol table node") != b"SNOD":
            raise ValueError(f"hdf5: symbol table node at offset {addr:#x} lacks its SNOD signature")
        n = f.u(addr + 6, 2, "SNOD symbol count")
        esize = 2 * self.O + 24
        f.need(addr + 8, n * esize, "SNOD entries")
        for i in range(n):
            e = addr + 8 + i * esize
            name = self._heap_name(heap, f.u(e, self.O, "link name offset"), e)
            target = self.addr(e + self.O, "object header address")
            if target is None:
                raise ValueError(f"hdf5: symbol table entry at offset {e:#x} has an undefined object address")
            out[name] = target

    def _link(self, p: int, n: int) -> Tuple[bytes, Optional[int]]:
        f = self.f
        end = p + n
        ver = f.u(p, 1, "link message version")
        if ver != 1:
            raise ValueError(f"hdf5: link message at offset {p:#x}: version {ver} (1 expected)")
        flags = f.u(p + 1, 1, "link message flags")
        q = p + 2
        ltype = 0
        if flags & 0x08:
            ltype = f.u(q, 1, "link type")
            q += 1
        if flags & 0x04:
            q += 8
        if flags & 0x10:
            q += 1
        w = 1 << (flags & 3)
        nlen = f.u(q, w, "link name length")
        q += w
        name = f.raw(q, nlen, "link name")
        q += nlen
        if q > end:
            raise ValueError(f"hdf5: link message at offset {p:#x} overruns its {n} bytes")
        if ltype != 0:
            return name, None                       # soft / external links are not followed
        return name, self.addr(q, "hard link address")

    # ---------------------------------------------------------------- datasets
    def dataset(self, o: _Obj) -> np.ndarray:
        shape = self._dataspace(o)
        dtype = self._datatype(o)
        lay = o.find(_LAYOUT)
        _t, _fl, p, n = lay[0]
        f = self.f
        ver = f.u(p, 1, "layout message version")
        if ver != 3:
            raise ValueError(f"hdf5: data layout message at offset {p:#x}: version {ver} (3 expected)")
        cls = f.u(p + 1, 1, "layout class")
        count = int(np.prod(shape, dtype=object)) if shape else 1
        nbytes = count * dtype.itemsize
        if cls == 0:
            size = f.u(p + 2, 2, "compact data size")
            if size < nbytes or 4 + size > n:
                raise ValueError(f"hdf5: compact layout at offset {p:#x}: {size} bytes stored for a "
                                 f"{nbytes}-byte dataset")
            return self._array(f.raw(p + 4, nbytes, "compact data"), dtype, shape)
        if cls == 1:
            a = self.addr(p + 2, "contiguous data address")
            size = f.u(p + 2 + self.O, self.L, "contiguous data size")
            if a is None:
                self._check_alloc(nbytes, p)
                return np.zeros(shape, dtype)
            if size < nbytes:
                raise ValueError(f"hdf5: contiguous layout at offset {p:#x}: {size} bytes stored for a "
                                 f"{nbytes}-byte dataset")
            return self._array(f.raw(a, nbytes, "contiguous data"), dtype, shape)
        if cls == 2:
            return self._chunked(o, p, n, shape, dtype, nbytes)
        raise ValueError(f"hdf5: data layout class {cls} at offset {p:#x} is not supported")

    def _check_alloc(self, nbytes: int, p: int) -> None:
        if nbytes > max(64 * self.f.n, 1 << 24):
            raise ValueError(f"hdf5: dataset described at offset {p:#x} would need {nbytes} bytes, "
                             f"implausible for a {self.f.n}-byte file")

    @staticmethod
    def _array(raw: bytes, dtype: np.dtype, shape: Tuple[int, ...]) -> np.ndarray:
        return np.frombuffer(raw, dtype=dtype).reshape(shape).astype(dtype.newbyteorder("="))

    def _dataspace(self, o: _Obj) -> Tuple[int, ...]:
        ds = o.find(_DATASPACE)
        if not ds:
            raise ValueError(f"hdf5: dataset at offset {o.addr:#x} has no dataspace message")
        _t, fl, p, n = ds[0]
        f = self.f
        if fl & 0x02:
            raise ValueError(f"hdf5: dataspace at offset {p:#x} is a shared message: not supported")
        ver = f.u(p, 1, "dataspace version")
        rank = f.u(p + 1, 1, "dataspace rank")
        if rank > _MAX_RANK:
            raise ValueError(f"hdf5: dataspace at offset {p:#x}: rank {rank}")
        if ver == 1:
            q = p + 8
        elif ver == 2:
            kind = f.u(p + 3, 1, "dataspace type")
            if kind == 2:
                raise ValueError(f"hdf5: dataspace at offset {p:#x} is null: not supported")
            if kind not in (0, 1):
                raise ValueError(f"hdf5: dataspace at offset {p:#x}: type {kind}")
            q = p + 4
        else:
            raise ValueError(f"hdf5: dataspace message at offset {p:#x}: version {ver} (1 or 2 expected)")
        if q + rank * self.L > p + n:
            raise ValueError(f"hdf5: dataspace at offset {p:#x} overruns its {n} bytes")
        return tuple(f.u(q + i * self.L, self.L, "dimension size") for i in range(rank))

    def _datatype(self, o: _Obj) -> np.dtype:
        dt = o.find(_DATATYPE)
        if not dt:
            raise ValueError(f"hdf5: dataset at offset {o.addr:#x} has no datatype message")
        _t, fl, p, n = dt[0]
        f = self.f
        if fl & 0x02:
            raise ValueError(f"hdf5: datatype at offset {p:#x} is shared (committed): not supported")
        cv = f.u(p, 1, "datatype class")
        cls, bits, size = cv & 0x0F, f.u(p + 1, 3, "datatype bit field"), f.u(p + 4, 4, "datatype size")
        if n < 12:
            raise ValueError(f"hdf5: datatype message at offset {p:#x} is {n} bytes long")
        off, prec = f.u(p + 8, 2, "bit offset"), f.u(p + 10, 2, "bit precision")
        if cls == 0:
            if size not in (1, 2, 4, 8) or off != 0 or prec != 8 * size:
                raise ValueError(f"hdf5: integer datatype at offset {p:#x}: size {size}, offset {off}, "
                                 f"precision {prec} (plain 8/16/32/64-bit integers are supported)")
            order = ">" if bits & 1 else "<"
            return np.dtype(f"{order}{'i' if bits & 0x08 else 'u'}{size}")
        if cls == 1:
            if n < 20:
                raise ValueError(f"hdf5: float datatype message at offset {p:#x} is {n} bytes long")
            layout = {2: (15, 10, 5, 0, 10, 15), 4: (31, 23, 8, 0, 23, 127), 8: (63, 52, 11, 0, 52, 1023)}
            got = (f.u(p + 2, 1, "sign location"), f.u(p + 12, 1, "exponent location"),
                   f.u(p + 13, 1, "exponent size"), f.u(p + 14, 1, "mantissa location"),
                   f.u(p + 15, 1, "mantissa size"), f.u(p + 16, 4, "exponent bias"))
            if bits & 0x40 or size not in layout or got != layout[size] or off != 0 or prec != 8 * size:
                raise ValueError(f"hdf5: float datatype at offset {p:#x}: size {size}, layout {got} "
                                 "(IEEE half/single/double are supported)")
            return np.dtype(f"{'>' if bits & 1 else '<'}f{size}")
        raise ValueError(f"hdf5: datatype class {cls} at offset {p:#x} is not supported "
                         "(integers and IEEE floats are)")

    def _chunked(self, o: _Obj, p: int, n: int, shape, dtype: np.dtype, nbytes: int) -> np.ndarray:
        f = self.f
        for _t, _fl, q, _n in o.find(_FILTERS):
            nf = f.u(q + 1, 1, "filter count")
            if nf:
                raise ValueError(f"hdf5: dataset at offset {o.addr:#x} has {nf} filter(s) "
                                 "(compressed/filtered chunks are not supported)")
        dims = f.u(p + 2, 1, "chunk dimensionality")
        if dims != len(shape) + 1 or 3 + self.O + 4 * dims > n:
            raise ValueError(f"hdf5: chunked layout at offset {p:#x}: dimensionality {dims} for a "
                             f"rank-{len(shape)} dataset")
        btree = self.addr(p + 3, "chunk B-tree address")
        cdims = [f.u(p + 3 + self.O + 4 * i, 4, "chunk dimension") for i in range(dims)]
        if cdims[-1] != dtype.itemsize or 0 in cdims:
            raise ValueError(f"hdf5: chunked layout at offset {p:#x}: chunk dims {cdims} for "
                             f"{dtype.itemsize}-byte elements")
        self._check_alloc(nbytes, p)
        out = np.zeros(shape, dtype)
        if btree is not None:
            self._chunk_btree(btree, out, cdims[:-1], dtype, set(), None)
        return out.astype(dtype.newbyteorder("="))

    def _chunk_btree(self, addr: int, out: np.ndarray, cdims: List[int], dtype, seen: set,
                     level: Optional[int]) -> None:
        f = self.f
        if addr in seen:
            raise ValueError(f"hdf5: chunk B-tree node at offset {addr:#x} is reached twice (cycle)")
        seen.add(addr)
        if f.raw(addr, 4, "chunk B-tree node") != b"TREE":
            raise ValueError(f"hdf5: chunk B-tree node at offset {addr:#x} lacks its TREE signature")
        ntype, lvl = f.u(addr + 4, 1, "B-tree node type"), f.u(addr + 5, 1, "B-tree node level")
        used = f.u(addr + 6, 2, "B-tree entries used")
        if ntype != 1 or (level is not None and lvl != level) or lvl > _MAX_DEPTH:
            raise ValueError(f"hdf5: chunk B-tree node at offset {addr:#x}: type {ntype}, level {lvl}")
        rank = out.ndim
        ksize = 8 + 8 * (rank + 1)
        p = addr + 8 + 2 * self.O
        f.need(p, used * (ksize + self.O) + ksize, "chunk B-tree entries")
        csize = int(np.prod(cdims, dtype=object)) * dtype.itemsize
        for i in range(used):
            k = p + i * (ksize + self.O)
            child = self.addr(k + ksize, "chunk address")
            if child is None:
                raise ValueError(f"hdf5: chunk B-tree node at offset {addr:#x}: child {i} is undefined")
            if lvl > 0:
                self._chunk_btree(child, out, cdims, dtype, seen, lvl - 1)
                continue
            stored, mask = f.u(k, 4, "chunk size"), f.u(k + 4, 4, "chunk filter mask")
            offs = [f.u(k + 8 + 8 * d, 8, "chunk offset") for d in range(rank)]
            if stored != csize or mask:
                raise ValueError(f"hdf5: chunk key at offset {k:#x}: {stored} bytes, filter mask {mask:#x} "
                                 f"({csize} unfiltered bytes expected)")
            if any(o_ % c or o_ >= s for o_, c, s in zip(offs, cdims, out.shape)):
                raise ValueError(f"hdf5: chunk key at offset {k:#x}: offsets {offs} do not fit dataset "
                                 f"{out.shape} with chunks {cdims}")
            chunk = np.frombuffer(f.raw(child, csize, "chunk data"), dtype=dtype).reshape(cdims)
            dst = tuple(slice(o_, min(o_ + c, s)) for o_, c, s in zip(offs, cdims, out.shape))
            out[dst] = chunk[tuple(slice(0, s.stop - s.start) for s in dst)]

    # ------------------------------------------------------------------- walks
    def walk(self) -> Iterator[Tuple[str, List[str], List[str]]]:
        stack = [("", self.root, (self.root,))]
        while stack:
            path, addr, chain = stack.pop()
            groups, dsets = [], []
            for name, child in self.members(self.obj(addr)):
                o = self.obj(child)
                if self.is_group(o):
                    if child in chain or len(chain) > _MAX_DEPTH:
                        raise ValueError(f"hdf5: group {path + '/' + name!r} at offset {child:#x} "
                                         "contains itself (cycle) or nests too deep")
                    groups.append(name)
                elif self.is_dataset(o):
                    dsets.append(name)
            yield path, groups, dsets
            o_members = dict(self.members(self.obj(addr)))
            for g in reversed(groups):
                child = o_members[g]
                stack.append((f"{path}/{g}" if path else g, child, chain + (child,)))

    def read_all(self) -> Dict[str, np.ndarray]:
        out: Dict[str, np.ndarray] = {}
        for path, _groups, dsets in self.walk():
            members = dict(self.members(self.obj(self._resolve(path))))
            for d in dsets:
                out[f"{path}/{d}" if path else d] = self.dataset(self.obj(members[d]))
        return out

    def _resolve(self, path: str) -> int:
        addr = self.root
        for part in [p for p in path.split("/") if p]:
            addr = dict(self.members(self.obj(addr)))[part]
        return addr


def _load(src: Union[str, Path, bytes, bytearray, memoryview]) -> _Reader:
    if isinstance(src, (bytes, bytearray, memoryview)):
        data = bytes(src)
    else:
        data = Path(src).read_bytes()
    return _Reader(data)


def _guarded(fn):
    """A malformed file that slips past the explicit checks still ends in a ValueError."""
    def wrap(*a, **k):
        try:
            return fn(*a, **k)
        except ValueError:
            raise
        except (IndexError, KeyError, struct.error, OverflowError, RecursionError, TypeError,
                MemoryError) as e:
            raise ValueError(f"hdf5: malformed file ({type(e).__name__}: {e})") from e
    wrap.__name__, wrap.__doc__ = fn.__name__, fn.__doc__
    return wrap


@_guarded
def read(src) -> Dict[str, np.ndarray]:
    """Every dataset in the file as {"group/sub/name": ndarray} (native byte order)."""
    return _Reader.read_all(_load(src))


@_guarded
def walk(src) -> List[Tuple[str, List[str], List[str]]]:
    """[(group path, subgroup names, dataset names)] top-down, like os.walk; the root is ""."""
    return list(_load(src).walk())


# ====================================================================== writer
_O = _L = 8
_UNDEF = b"\xff" * 8
_INTERNAL_K = 16


def _pad8(b: bytes) -> bytes:
    return b + b"\0" * (-len(b) % 8)


def _msg(mtype: int, data: bytes, flags: int = 0) -> bytes:
    data = _pad8(data)
    return struct.pack("<HHB3x", mtype, len(data), flags) + data


def _ohdr_v1(msgs: List[bytes]) -> bytes:
    body = b"".join(msgs)
    return struct.pack("<BBHII4x", 1, 0, len(msgs), 1, len(body)) + body


def _dtype_msg(dt: np.dtype) -> bytes:
    if dt.kind == "f":
        sign, eloc, esz, msz, bias = {2: (15, 10, 5, 10, 15), 4: (31, 23, 8, 23, 127),
                                      8: (63, 52, 11, 52, 1023)}[dt.itemsize]
        head = struct.pack("<B3BI", 0x11, 0x20, sign, 0, dt.itemsize)
        return head + struct.pack("<HHBBBBI", 0, 8 * dt.itemsize, eloc, esz, 0, msz, bias)
    head = struct.pack("<B3BI", 0x10, 0x08 if dt.kind == "i" else 0, 0, 0, dt.itemsize)
    return head + struct.pack("<HH", 0, 8 * dt.itemsize)


class _Writer:
    def __init__(self, tree: dict) -> None:
        self.k = max(4, math.ceil(self._widest(tree) / 2))
        self.buf = bytearray(96)                    # superblock, patched last

    @staticmethod
    def _widest(tree: dict) -> int:
        w = len(tree)
        for v in tree.values():
            if isinstance(v, dict):
                w = max(w, _Writer._widest(v))
        return w

    def put(self, data: bytes) -> int:
        self.buf += b"\0" * (-len(self.buf) % 8)
        at = len(self.buf)
        self.buf += data
        return at

    def dataset(self, arr: np.ndarray) -> int:
        arr = np.asarray(arr)
        if arr.dtype.kind not in "fiu" or (arr.dtype.kind == "f" and arr.dtype.itemsize not in (2, 4, 8)) \
                or arr.dtype.itemsize not in (1, 2, 4, 8):
            raise ValueError(f"hdf5.write: dtype {arr.dtype} is outside the supported subset")
        if arr.ndim > _MAX_RANK:
            raise ValueError(f"hdf5.write: rank {arr.ndim}")
        raw = np.ascontiguousarray(arr, dtype=arr.dtype.newbyteorder("<")).tobytes()
        addr = self.put(raw) if raw else None
        space = struct.pack("<BBBx4x", 1, arr.ndim, 0) + b"".join(struct.pack("<Q", d) for d in arr.shape)
        fill = struct.pack("<BBBB", 2, 2, 2, 0)
        layout = struct.pack("<BB", 3, 1) + (_UNDEF if addr is None else struct.pack("<Q", addr)) \
            + struct.pack("<Q", len(raw))
        return self.put(_ohdr_v1([_msg(_DATASPACE, space), _msg(_DATATYPE, _dtype_msg(arr.dtype), 1),
                                  _msg(_FILL, fill, 1), _msg(_LAYOUT, layout)]))

    def group(self, tree: dict) -> Tuple[int, int, int]:
        """-> (object header, B-tree, local heap) addresses."""
        entries = []
        for name in sorted(tree, key=lambda s: s.encode("utf-8")):
            if not name or "/" in name or "." == name:
                raise ValueError(f"hdf5.write: bad member name {name!r}")
            v = tree[name]
            if isinstance(v, dict):
                oh, bt, hp = self.group(v)
                entries.append((name, oh, 1, struct.pack("<QQ", bt, hp)))
            else:
                entries.append((name, self.dataset(v), 0, b"\0" * 16))
        heap = bytearray(8)                          # offset 0: the empty name
        offs = []
        for name, *_ in entries:
            offs.append(len(heap))
            heap += _pad8(name.encode("utf-8") + b"\0")
        heap_addr = len(self.buf) + (-len(self.buf) % 8)
        heap_addr = self.put(b"HEAP" + struct.pack("<B3xQQQ", 0, len(heap), 1, heap_addr + 32) + bytes(heap))
        esize = 2 * _O + 24
        snod_size = 8 + 2 * self.k * esize
        node_size = 8 + 2 * _O + 2 * _INTERNAL_K * _O + (2 * _INTERNAL_K + 1) * _L
        if entries:
            snod = b"SNOD" + struct.pack("<BxH", 1, len(entries)) + b"".join(
                struct.pack("<QQII", off, oh, cache, 0) + scratch
                for off, (_n, oh, cache, scratch) in zip(offs, entries))
            snod_addr = self.put(snod + b"\0" * (snod_size - len(snod)))
            tree_node = b"TREE" + struct.pack("<BBH", 0, 0, 1) + _UNDEF + _UNDEF \
                + struct.pack("<QQQ", 0, snod_addr, offs[-1])
        else:
            tree_node = b"TREE" + struct.pack("<BBH", 0, 0, 0) + _UNDEF + _UNDEF + struct.pack("<Q", 0)
        bt_addr = self.put(tree_node + b"\0" * (node_size - len(tree_node)))
        oh = self.put(_ohdr_v1([_msg(_STAB, struct.pack("<QQ", bt_addr, heap_addr))]))
        return oh, bt_addr, heap_addr

    def finish(self, tree: dict) -> bytes:
        root, bt, hp = self.group(tree)
        self.buf += b"\0" * (-len(self.buf) % 8)
        sb = SIGNATURE + struct.pack("<BBBBBBBB", 0, 0, 0, 0, 0, _O, _L, 0) \
            + struct.pack("<HHI", self.k, _INTERNAL_K, 0) \
            + struct.pack("<Q", 0) + _UNDEF + struct.pack("<Q", len(self.buf)) + _UNDEF \
            + struct.pack("<QQII", 0, root, 1, 0) + struct.pack("<QQ", bt, hp)
        assert len(sb) == 96
        self.buf[:96] = sb
        return bytes(self.buf)


def write(dst: Union[str, Path, io.IOBase, None], tree: dict) -> bytes:
    """Write `tree` (nested dicts = groups, arrays = datasets) as an HDF5 file; returns its bytes
    and, when `dst` is a path or a binary file object, stores them there too."""
    data = _Writer(tree).finish(tree)
    if isinstance(dst, (str, Path)):
        Path(dst).write_bytes(data)
    elif dst is not None:
        dst.write(data)
    return data


def nest(flat: Dict[str, np.ndarray]) -> dict:
    """{"a/b/c": arr} -> {"a": {"b": {"c": arr}}} (the inverse of `read`'s flattening)."""
    tree: dict = {}
    for path, arr in flat.items():
        node = tree
        parts = path.split("/")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
            if not isinstance(node, dict):
                raise ValueError(f"hdf5.nest: {path!r} runs through a dataset")
        node[parts[-1]] = arr
    return tree
