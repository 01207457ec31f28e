"""Files -> resized uint8 batches in HBM: the decode step either side of every kernel.

The reference decodes one file after the other with Pillow and resizes on the host
(`ImageLoader.load_as_array` / `resize_array`, srcs/utils/image_utils.py:19-59,109-114, called from
srcs/dataio/sequence.py:74-125 and srcs/predict/predictor.py).  Here codec worker processes read the
files and, of baseline 4:2:0 JPEGs of any height and any width from 5 up, either the markers only (`chunks`: the
un-stuffed scan goes into the page-locked slab and the GPU decodes the Huffman stream too, `ops.jpeg_huffman_u8`) or the
markers and the Huffman stream (the prefetching `submit` / `collect`, which never waits for the GPU and so cannot ask it
for a verdict on a damaged scan); any other file (grey, other samplings, progressive, narrower than 5 pixels) is decoded
whole by Pillow in the worker.  A chunk crosses PCIe as one copy (its used parts only when every file is a prepared
scan), and the GPU does dequantisation / IDCT / fancy upsampling / colour conversion and the Pillow-exact LANCZOS
resize, chunk after chunk with the next two chunks' files already being read.  A chunk of one whole-MCU size goes
through the one-size calls, any other through the `_items_` calls (`route_slots`): one Huffman, one IDCT, one upsampling
and one LANCZOS launch for all its sizes (`ops.resize_lanczos_items_u8` reads the pixel buffer where the upsampling
left it and writes the batch's rows; the Pillow-decoded slots of such a chunk are a second call over the staging
buffer).  The pixels are Pillow's bit for bit (tests/test_jpeg_codec.py, tests/test_jpeg_ragged.py), so everything
downstream sees what the reference's loop would have produced.  `counts` says how the files were decoded.
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np


# ---- One chunk of codec-worker slots on the device, for this loader and the balancer's GPU stage.  `decoded[k]` is what
# the worker left in slot k, (status, payload, params): "scan" (a prepared scan: payload = (h, w, table hash, used
# bytes)), "coef" (Huffman-decoded on the host: (h, w, ...)), "ok" (Pillow's pixels), "big" or "err".
def upload_ranges(decoded: Sequence[tuple], slot: int) -> Optional[List[Tuple[int, int]]]:
    """The byte ranges of every slot that have to cross PCIe, or None for whole slots: when every live slot is a prepared
    scan, the quantisation tables at the front and, behind the (device-only) coefficient area, header / Huffman tables /
    scan up to the longest one's end — ~27 KB of a 301 KB slot for a 224 x 224 file."""
    from ..utils import jpeg_host
    live = [d for d in decoded if d[0] != "err"]
    if not live or any(d[0] != "scan" for d in live):
        return None
    lo = min(jpeg_host.scan_aux_offset_ragged(h, w) for h, w in {(d[1][0], d[1][1]) for d in live})
    hi = (max(d[1][3] for d in live) + 15) // 16 * 16
    return [(0, 256), (lo, hi)] if 256 <= lo < hi <= slot else None


def upload_slots(dev_in, host, n: int, slot: int, decoded: Sequence[tuple], pinned: bool = True) -> None:
    """Slots [0, n) of the slab run `host` -> rows [0, n) of the device mirror `dev_in`, queued on the current stream:
    `upload_ranges` as row copies (hipMemcpy2DAsync out of the page-locked slab; torch's own strided copy goes through
    a pageable temporary and measured 8x slower than whole slots), else whole slots in one contiguous copy."""
    import torch

    from .. import _lib
    ranges = upload_ranges(decoded, slot) if pinned else None
    if ranges is None:
        dev_in[:n].copy_(host if pinned else host.clone(), non_blocking=pinned)
    for lo, hi in ranges or []:
        _lib.call("lf_copy_rows", dev_in.data_ptr() + lo, slot, host.data_ptr() + lo, slot, hi - lo, n, 0,
                  torch.cuda.current_stream().cuda_stream)


def route_slots(decoded: Sequence[tuple]) -> Tuple[List[int], bool]:
    """(positions of the JPEG slots, "scan" or "coef", in order; whether they take the `_items_` calls).  One whole-MCU
    size and one kind: the one-size calls.  Several, or a size that is not whole MCUs (a tree that was augmented before:
    every rotated canvas has a size of its own): decoded where they lie, all in one launch per step."""
    jpeg = [k for k, d in enumerate(decoded) if d[0] in ("scan", "coef")]
    kinds = {(decoded[k][0],) + tuple(decoded[k][1][:2]) for k in jpeg}
    return jpeg, len(kinds) > 1 or any(h % 16 or w % 16 for _st, h, w in kinds)


def device_index(ks: Sequence[int], dev, pinned: bool = True):
    """`ks` as an int64 index tensor on the device, without waiting for it."""
    import torch
    t = torch.tensor(ks, dtype=torch.int64)
    return (t.pin_memory() if pinned else t).to(dev, non_blocking=pinned)


class DecodedSlots:
    """What `decode_slots` queued for the positions `jpeg`.  `huffman`: [(positions, device status of the GPU's Huffman
    decoding)], not waited for; non-zero is a scan handed back (damaged, cut short: Pillow has the reference's verdict).
    One-size route: `px` is [len(jpeg), h, w, 3], row j = position jpeg[j], `index` the device index of `jpeg` (None:
    the whole chunk).  Items route (`mixed`): `px` is the flat pixel buffer, `items` the JpegDecItems whose offsets[j]
    and sizes[j] say where position jpeg[j]'s pixels lie, `views[j]` their [h, w, 3] view."""

    def __init__(self, jpeg: List[int], mixed: bool) -> None:
        self.jpeg, self.mixed, self.huffman = jpeg, mixed, []
        self.px = self.index = self.items = self.views = None


def decode_slots(dev_in, slot: int, decoded: Sequence[tuple], pinned: bool = True) -> DecodedSlots:
    """The JPEG back end over the uploaded mirror `dev_in` ([>= len(decoded), slot] uint8): Huffman decoding of the
    "scan" slots, then dequantisation / IDCT / upsampling / colour conversion of all JPEG slots, by `route_slots`' route.
    Nothing here waits for the GPU."""
    from .. import ops
    out = DecodedSlots(*route_slots(decoded))
    jpeg, n = out.jpeg, len(decoded)
    scans = [k for k in jpeg if decoded[k][0] == "scan"]
    if out.mixed:
        flat = dev_in.view(-1)
        item = [(k * slot, slot) + tuple(decoded[k][1][:2]) for k in jpeg]
        if scans:
            out.huffman.append((scans, ops.jpeg_huffman_items_u8(flat, [it for k, it in zip(jpeg, item) if decoded[k][0] == "scan"])))
        out.items = ops.JpegDecItems(item, dev_in.device)
        out.px, out.views = ops.jpeg_idct_rgb_items_u8(flat, out.items)
    elif jpeg:
        h, w = decoded[jpeg[0]][1][:2]
        if len(jpeg) < n:   # (else they are the whole chunk, the usual case: no gather)
            out.index = device_index(jpeg, dev_in.device, pinned)
        rows = dev_in[:n] if out.index is None else dev_in[out.index]
        if scans:
            out.huffman.append((jpeg, ops.jpeg_huffman_u8(rows, h, w)))
        out.px = ops.jpeg_idct_rgb_u8(rows, h, w)
    return out


class DeviceDecoder:
    """`chunks(paths, img_size)` yields `(first, kept, x, natives, errors)` per chunk of up to `CHUNK` files:
    `kept` = positions (into `paths`) that decoded, in order; `x` = uint8 device tensor [len(kept), S, S, 3];
    `natives` = the decoded images at their own size (host arrays, `keep_native=True` only, else None);
    `errors` = [(position, message)] for the files that did not decode.  The worker processes and their
    slabs live until `close()`: starting them costs as much as decoding a thousand files.
    `submit(paths, img_size)` / `collect(handle)` split one batch into its worker half and its device half, so a
    loader can have the next batch's files decoding while the current one trains."""

    CHUNK = 256

    def __init__(self, workers: Optional[int] = None) -> None:
        from ..utils.system_info import get_optimal_worker_count
        self.workers = int(workers or get_optimal_worker_count())   # (already the rank's share of the node's cores)
        self._codec = None   # (CodecPool, slot_bytes, pinned, device staging)
        self._pending: List[dict] = []   # submitted, not yet collected batches (at most two)
        self._uploaded = [None, None, None]   # per slab third: event behind its last (asynchronous) upload
        self._ring = 0                   # next slab third `submit` uses
        # how the files were decoded so far: Huffman and pixels on the GPU | Huffman in the worker, pixels on the GPU |
        # whole by Pillow (in the worker, or here for a scan the GPU handed back) | by Pillow, too large for the slot
        # and so pickled | not at all (an error)
        self.counts: Dict[str, int] = {"gpu_huffman": 0, "host_huffman": 0, "pillow": 0, "pickled": 0, "failed": 0}

    def _ensure(self, slot: int):
        import torch

        from ..preprocessing.codec_pool import CodecPool
        if self._codec is not None and self._codec[1] < slot:
            self.close()
        if self._codec is None:
            pool = CodecPool(self.workers)
            pool.allocate(3 * self.CHUNK, slot)
            dev = torch.device("cuda", torch.cuda.current_device())
            self._codec = (pool, slot, pool.pin(), torch.empty((self.CHUNK, slot), dtype=torch.uint8, device=dev))
        return self._codec

    @staticmethod
    def _probe_slot(paths: Sequence[str], fallback: int, scan: bool = False, samples: int = 32) -> int:
        """Slot size from the largest of `samples` files spread evenly over the list (their headers only), by its
        padded footprint: the coefficients of a size that is not whole MCUs are those of ceil(h/16) * ceil(w/16) MCUs.
        Not from the first file: in an augmented tree the first files of a class folder may all be originals while a
        +-30 degree rotate(expand=True) canvas has up to (cos 30 + sin 30)^2 = 1.87 times their area.  Only the used
        front of a slot crosses PCIe, so a larger slot costs page-locked memory, not transfer.  A canvas that still
        does not fit — larger than everything sampled — is decoded whole by Pillow in the worker and travels as a
        pickled array (counted as "pickled"): ~0.6 ms of a worker and ten times the bytes, but the same pixels."""
        from PIL import Image
        px, seen = fallback * fallback, 0
        last = len(paths) - 1
        spread = sorted({round(j * last / max(1, samples - 1)) for j in range(samples)}) if last > 0 else [0]
        for p in (paths[j] for j in spread[:len(paths)]):
            try:
                with Image.open(p) as probe:
                    w0, h0 = probe.size
            except Exception:  # noqa: BLE001
                continue
            px = max(px if seen else 0, 256 * -(-h0 // 16) * -(-w0 // 16))
            seen += 1
        # tables + coefficients (or pixels), and behind them room for a prepared scan (header, Huffman tables and the
        # un-stuffed entropy-coded bytes: ~0.16 of the pixel bytes at quality 95; a file that does not fit takes the
        # host's Huffman pass)
        return (256 + px * 3 + ((1136 + px * 3 // 2) if scan else 0) + 4095) // 4096 * 4096

    def _submit(self, part: Sequence[str], third: int, scan: bool = False):
        """`scan`: the workers read the markers only and the GPU decodes the Huffman stream as well — for callers that
        can wait for the chunk's GPU work before they use its pixels (`chunks`); the prefetching path (`submit` /
        `collect`, which never waits) keeps the Huffman pass in the workers."""
        pool = self._codec[0]
        ev = self._uploaded[third]   # the last upload out of this slab third must be over before it is rewritten
        if ev is not None:
            ev.synchronize()
            self._uploaded[third] = None
        tasks = [{"source_img": p, "transform_name": "", "seed": 0} for p in part]
        # every future costs the parent ~0.1-0.2 ms to send and collect: one job per worker for a small batch (a
        # 32-file batch as 32 one-file jobs ran at half the rate), two for a full chunk (some slack for a slow core)
        return pool.decode(tasks, third * self.CHUNK, 2 if scan else 1, pieces_per_worker=1 if len(part) <= 64 else 2)

    def _finish(self, futures, third: int, n: int, img_size: int, keep_native: bool, pos0: int,
                paths: Optional[Sequence[str]] = None):
        """The device half of one chunk whose worker jobs are `futures`: upload, the JPEG back end, the resize, the
        scans the GPU handed back.  Returns (kept positions, x, natives, errors); the slab third is free again once
        `_uploaded[third]` has passed."""
        import torch
        pool, slot, pinned, dev_in = self._codec
        decoded = [r for f in futures for r in f.result()]
        host = pool.tensor("in", third * self.CHUNK, n)
        # Nothing below waits for the GPU (unless `keep_native` fetches pixels back) before the hand-backs: the device
        # half queues behind whatever the stream is doing — a training step — and the host goes on to prepare the next
        # one.  The one staging buffer is safe to reuse: uploads and the kernels that read it are ordered on the stream.
        dev_in = dev_in[:n]
        upload_slots(dev_in, host, n, slot, decoded, pinned)
        if pinned:
            ev = torch.cuda.Event()
            ev.record()
            self._uploaded[third] = ev
        dec = decode_slots(dev_in, slot, decoded, pinned)
        x, kept, natives, errors = self._resize_scatter(decoded, dec, dev_in, host, int(img_size), pos0, keep_native)
        self._hand_backs(dec.huffman, paths, int(img_size), pos0, x, kept, natives, errors)
        if len(kept) < n:
            x = x[device_index(kept, x.device, pinned)] if kept else x[:0]
        return [pos0 + k for k in kept], x, natives, errors

    def _resize_scatter(self, decoded, dec: DecodedSlots, dev_in, host, S: int, pos0: int, keep_native: bool):
        """Every decoded slot's pixels, resized, into its row of the batch `x` [n, S, S, 3]; `counts` and the workers'
        errors on the way.  Returns (x, positions that have pixels, natives, errors)."""
        import torch

        from .. import ops
        _pool, slot, pinned, _dev = self._codec
        n, dev, counts = len(decoded), dev_in.device, self.counts
        # The JPEG slots of the items route are resized from where the upsampling left them, all sizes in one launch;
        # so are the Pillow-decoded slots ("ok") of such a chunk, or of several sizes.  Anything else goes by size.
        plain = [k for k, d in enumerate(decoded) if d[0] == "ok"]
        if not dec.mixed and len({tuple(decoded[k][1][:2]) for k in plain}) <= 1:
            plain = []
        groups: Dict[tuple, List[int]] = {}
        big: Dict[int, np.ndarray] = {}
        errors: List[Tuple[int, str]] = []
        for k, (status, payload, _prm) in enumerate(decoded):
            if status == "err":
                errors.append((pos0 + k, payload))
                counts["failed"] += 1
            elif status == "big":
                big[k] = payload
                groups.setdefault(("big",) + tuple(payload.shape[:2]), []).append(k)
                counts["pickled"] += 1
            else:
                if not ((dec.mixed and status in ("scan", "coef")) or (plain and status == "ok")):
                    groups.setdefault((status,) + tuple(payload[:2]), []).append(k)
                counts[{"scan": "gpu_huffman", "coef": "host_huffman", "ok": "pillow"}[status]] += 1
        natives: Optional[Dict[int, np.ndarray]] = {} if keep_native else None
        x = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
        if dec.mixed:
            where = [(o, hh, ww) for o, (hh, ww) in zip(dec.items.offsets, dec.items.sizes)]
            ops.resize_lanczos_items_u8(dec.px, where, S, out=x, out_index=dec.jpeg)
            if natives is not None:
                host_buf = dec.px.cpu().numpy()
                for k, (o, hh, ww) in zip(dec.jpeg, where):
                    natives[pos0 + k] = host_buf[o:o + 3 * hh * ww].reshape(hh, ww, 3)
        if plain:   # Pillow's pixels lie at the front of their slots
            ops.resize_lanczos_items_u8(dev_in.view(-1), [(k * slot,) + tuple(decoded[k][1][:2]) for k in plain], S,
                                        out=x, out_index=plain)
            if natives is not None:
                for k in plain:
                    hh, ww = decoded[k][1][:2]
                    natives[pos0 + k] = host[k, :3 * hh * ww].reshape(hh, ww, 3).numpy().copy()
        for (status, h, w), ks in groups.items():
            whole = len(ks) == n   # one group holds the whole chunk (the usual case): no gather, no scatter
            if status in ("scan", "coef"):
                px, idx = dec.px, dec.index
            else:
                idx = None if whole else device_index(ks, dev, pinned)
                px = (dev_in if whole else dev_in[idx])[:, :h * w * 3].view(len(ks), h, w, 3) if status == "ok" else \
                    torch.from_numpy(np.stack([big[k] for k in ks])).to(dev)
            res = px if (h, w) == (S, S) else ops.resize_lanczos_u8(px.contiguous(), S)
            if whole:   # (a view of the staging buffer is never contiguous: it gets copied here)
                x = res if res.is_contiguous() else res.contiguous()
            else:
                x[idx] = res
            if natives is not None:
                host_px = px.cpu().numpy()
                for j, k in enumerate(ks):
                    natives[pos0 + k] = host_px[j]
        kept = sorted((dec.jpeg if dec.mixed else []) + plain + [k for ks in groups.values() for k in ks])
        return x, kept, natives, errors

    def _hand_backs(self, huffman, paths, S: int, pos0: int, x, kept: List[int], natives, errors) -> None:
        """A scan the GPU handed back goes to Pillow, which has the reference's verdict (image_utils.py:19-33): pixels,
        with libjpeg's concealment, into the file's row of `x`, or an error and the position out of `kept`.  Reading a
        status waits for the chunk's device half: only `chunks` asks for prepared scans."""
        import torch

        from .. import ops
        counts = self.counts
        for ks, st in huffman:
            for k in (k for k, v in zip(ks, st.cpu().numpy()) if v):
                counts["gpu_huffman"] -= 1
                counts["pillow"] += 1
                try:
                    from ..utils.image_utils import ImageLoader
                    arr = ImageLoader.load_as_array(paths[k])
                    one = torch.from_numpy(np.ascontiguousarray(arr)).to(x.device).unsqueeze(0)
                    x[k] = (one if tuple(arr.shape[:2]) == (S, S) else ops.resize_lanczos_u8(one, S))[0]
                    if natives is not None:
                        natives[pos0 + k] = arr
                except Exception as e:  # noqa: BLE001
                    errors.append((pos0 + k, f"{paths[k]} - {e}"))
                    counts["pillow"] -= 1
                    counts["failed"] += 1
                    kept.remove(k)
                    if natives is not None:
                        natives.pop(pos0 + k, None)

    def drop_pending(self) -> None:
        """Wait for (and drop) what `submit` left pending — the synchronous path is about to use every third, or
        the caller no longer wants those batches; `collect` on a dropped handle returns None."""
        for h in self._pending:
            h["dropped"] = True
            for f in h["futures"]:
                try:
                    f.result()
                except Exception:  # noqa: BLE001
                    pass
        self._pending = []
        self._ring = 0

    def chunks(self, paths: Sequence, img_size: int, keep_native: bool = False) -> Iterator[
            Tuple[int, List[int], "object", Optional[Dict[int, np.ndarray]], List[Tuple[int, str]]]]:
        C = self.CHUNK
        paths = [str(p) for p in paths]
        self.drop_pending()
        self._ensure(self._probe_slot(paths, int(img_size), scan=True))
        parts = [paths[b:b + C] for b in range(0, len(paths), C)]
        try:
            ahead = [self._submit(parts[i], i % 3, scan=True) for i in range(min(2, len(parts)))]
            for i, part in enumerate(parts):
                futures = ahead.pop(0)
                for f in futures:
                    f.result()
                if i + 2 < len(parts):   # into the slab third chunk i-1 used: its upload was waited for
                    ahead.append(self._submit(parts[i + 2], (i + 2) % 3, scan=True))
                kept, x, natives, errors = self._finish(futures, i % 3, len(part), img_size, keep_native, i * C, part)
                yield i * C, kept, x, natives, errors
        except BaseException:
            self.close()   # a failed chunk may leave jobs in flight on the slabs: start afresh next time
            raise

    # ---- one batch ahead: the worker half now, the device half when the batch is asked for
    def submit(self, paths: Sequence, img_size: int):
        """Start the worker half (file read + Huffman decoding) of one batch of at most CHUNK files and return a
        handle for `collect`, or None when two batches are already pending (the slab ring has three thirds)."""
        paths = [str(p) for p in paths]
        if not paths or len(paths) > self.CHUNK or len(self._pending) >= 2:
            return None
        slot = self._probe_slot(paths, int(img_size), samples=4)   # (per batch: four headers, not thirty-two)
        if self._codec is None or self._codec[1] < slot:
            self.drop_pending()
            self._ensure(slot)
        third = self._ring % 3
        self._ring += 1
        h = {"futures": self._submit(paths, third), "third": third, "n": len(paths), "S": int(img_size)}
        self._pending.append(h)
        return h

    def collect(self, h):
        """The device half of a submitted batch: (kept positions, uint8 device tensor [len(kept), S, S, 3], errors);
        None when the handle was dropped in the meantime."""
        if h.get("dropped") or not any(q is h for q in self._pending):
            return None
        try:
            kept, x, _nat, errors = self._finish(h["futures"], h["third"], h["n"], h["S"], False, 0)
        except BaseException:
            self.close()
            raise
        self._pending = [q for q in self._pending if q is not h]
        return kept, x, errors

    def close(self) -> None:
        """Stop the codec workers and release their slabs (idempotent)."""
        codec, self._codec = self._codec, None
        self._pending, self._ring = [], 0
        if codec is not None:
            import torch
            if any(ev is not None for ev in self._uploaded):
                torch.cuda.synchronize()   # uploads out of the slabs that are about to be unmapped
            self._uploaded = [None, None, None]
            codec[0].close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass
