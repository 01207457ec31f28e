"""Where to put the default Hamming threshold of the near-duplicate search: measured, not guessed.

  python scripts/duplicates_threshold.py [--images 800] [--out profiles/duplicates_threshold.json]

On the synthetic labelled leaves of `convergence.py` (`build_dataset`, 224 x 224 JPEGs at quality 95), hashed through
`dataio.duplicates.signatures` (DeviceDecoder -> nn.dhash128, variants = 2):
  (a) the distance between an image and its copies: re-saved at JPEG quality 60, 75, 85 and 95, and resized to 0.5x
      and to 2x (Pillow LANCZOS, saved at quality 95; the decoder brings them back to 224 x 224);
  (b) the distance between distinct images of the same class, all pairs.
A distance is the minimum over the two variants of the second image, as `nn.hamming_pairs` takes it.

The rule for the default: T = floor(2/3 of the closest distinct same-class pair found).  An all-pairs search over N
files of a class judges N^2 / 2 pairs, far more than the pairs of (b) measured here, so a share of (b) that looks small
is still a flood of false pairs (0.1 % of the pairs of 12,500 files are 78,000, and union-find chains them into one
group): the default has to lie below everything (b) shows, with a margin for the tail that a sample of this size
cannot show.  The default is useful if it keeps at least 90 % of (a).  Otherwise no default separates copies from
neighbours of the same class, and the default is 0 (exact-content twins only) with `--by both` recommended.  Both
histograms, the shares at every second threshold and the choice go to `--out` (histogram[d] = pairs at distance d, cut after
the last occupied bin)."""
import argparse
import json
import re
import shutil
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

QUALITIES = (60, 75, 85, 95)
SCALES = (0.5, 2.0)
MARGIN, KEEP_AT_LEAST = (2, 3), 0.9   # default = floor(2/3 of the closest distinct pair)


def derive(job):
    k, src, out_dir = job   # (the stems repeat from class to class: the copies are numbered)
    from PIL import Image
    made = []
    with Image.open(src) as im:
        im = im.convert("RGB")
        for q in QUALITIES:
            p = Path(out_dir) / f"{k:06d}_q{q}.jpg"
            im.save(p, quality=q)
            made.append((f"quality_{q}", str(p)))
        for s in SCALES:
            p = Path(out_dir) / f"{k:06d}_x{s}.jpg"
            im.resize((int(im.width * s), int(im.height * s)), Image.LANCZOS).save(p, quality=95)
            made.append((f"resize_{s}", str(p)))
    return made


_POP = np.array([bin(i).count("1") for i in range(1 << 16)], np.int32)


def distances(a, b):
    """a uint32 [n,4] (variant 0), b uint32 [n,V,4] -> int [n]: min over V of popcount(a xor b)."""
    x = a[:, None, :] ^ b
    return (_POP[x & 0xFFFF] + _POP[x >> 16]).sum(-1).min(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=800)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "duplicates_threshold.json")
    args = ap.parse_args()
    from concurrent.futures import ProcessPoolExecutor

    import convergence
    from leaffliction_amd.dataio import duplicates as D
    from leaffliction_amd.dataio.device_decode import DeviceDecoder
    work = Path(tempfile.mkdtemp(prefix="dup_threshold_"))
    try:
        manifest = convergence.build_dataset(work, args.images, 224)
        items = json.loads(manifest.read_text())["items"]
        originals = [it["src"] for it in items]
        labels = np.array([convergence.CLASSES.index(it["class"]) for it in items])
        copies = work / "copies"
        copies.mkdir()
        with ProcessPoolExecutor(max_workers=16) as ex:
            derived = list(ex.map(derive, [(k, p, str(copies)) for k, p in enumerate(originals)], chunksize=16))
        dec = DeviceDecoder()
        try:
            sig, kept, errors = D.signatures(originals, 224, 2, dec)
            assert kept == list(range(len(originals))) and not errors
            sig = sig.cpu().numpy().view(np.uint32)
            a_hist, by_kind = np.zeros(129, np.int64), {}
            for k, kind in enumerate([kind for kind, _p in derived[0]]):
                s2, kept2, errors2 = D.signatures([d[k][1] for d in derived], 224, 2, dec)
                assert kept2 == kept and not errors2
                d = distances(sig[:, 0], s2.cpu().numpy().view(np.uint32))
                by_kind[kind] = np.bincount(d, minlength=129)
                a_hist += by_kind[kind]
        finally:
            dec.close()
        b_hist = np.zeros(129, np.int64)
        for c in range(len(convergence.CLASSES)):
            s = sig[labels == c]
            i, j = np.triu_indices(len(s), 1)
            b_hist += np.bincount(distances(s[i, 0], s[j]), minlength=129)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    def cut(hist):
        return hist[:int(np.nonzero(hist)[0].max()) + 1].tolist()
    keep = np.cumsum(a_hist) / a_hist.sum()      # share of (a) within T
    admit = np.cumsum(b_hist) / b_hist.sum()     # share of (b) within T
    closest = int(np.nonzero(b_hist)[0].min())
    candidate = closest * MARGIN[0] // MARGIN[1]
    useful = bool(keep[candidate] >= KEEP_AT_LEAST)
    choice = candidate if useful else 0
    doc = {"dataset": {"generator": "scripts/convergence.py build_dataset", "images": len(originals), "size": 224,
                       "classes": len(convergence.CLASSES)},
           "variants": 2, "img_size": 224,
           "rule": {"default": "floor(2/3 * closest distinct same-class pair)", "keep_at_least_of_a": KEEP_AT_LEAST},
           "a_copies": {"pairs": int(a_hist.sum()), "max": int(np.nonzero(a_hist)[0].max()),
                        "histogram": cut(a_hist),
                        "by_kind": {k: {"max": int(np.nonzero(h)[0].max()), "mean": float((h * np.arange(129)).sum() / h.sum()),
                                        "histogram": cut(h)} for k, h in by_kind.items()}},
           "b_same_class": {"pairs": int(b_hist.sum()), "min": int(np.nonzero(b_hist)[0].min()),
                            "histogram": cut(b_hist)},
           "shares": [{"threshold": t, "keeps_of_a": round(float(keep[t]), 6), "admits_of_b": round(float(admit[t]), 6)}
                      for t in range(0, 65, 2)],
           "candidate": candidate, "useful": bool(useful), "default_threshold": choice,
           "keeps_of_a": float(keep[choice]), "admits_of_b": float(admit[choice])}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    # one line per entry, the lists (histograms cut after their last occupied bin) on one line each
    text = re.sub(r"\[\s+([^\[\]{}]*?)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]",
                  json.dumps(doc, indent=1))
    args.out.write_text(text + "\n")
    print(json.dumps({k: doc[k] for k in ("candidate", "useful", "default_threshold", "keeps_of_a", "admits_of_b")}))
    print(json.dumps({"a_max": doc["a_copies"]["max"], "b_min": doc["b_same_class"]["min"],
                      "a_by_kind_max": {k: v["max"] for k, v in doc["a_copies"]["by_kind"].items()}}))


if __name__ == "__main__":
    main()
