"""Near-duplicates end to end on the GPU: files -> DeviceDecoder -> dhash128 -> hamming_pairs -> groups, the
`duplicates` CLI's counts, and `split --group-duplicates` judged by that CLI.

The tree (Apple/healthy, Apple/rust; 64 x 64 JPEGs of smooth random patterns):
  10 + 10 distinct pictures h0..h9 / r0..r9;
  byte-identical copies under other names: healthy/copy_of_h0, healthy/zz_h1, and under the other label rust/h2_as_rust;
  mirrored re-saves under the balancer's names: h3_aug_flip_1, h4_aug_flip_1, r3_aug_flip_1 (the name rule groups them
  whatever JPEG rounding does to a bit; the hash rule finds them through variant 1).
"""
import json
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

import dups_ref as R

pytestmark = pytest.mark.gpu

SIZE = 64
T = 6
# `split` is host arithmetic once the groups are known, so the seed was chosen on the CPU with the groups this tree
# has by construction (equal bytes, balancer names): without the flag it parts copy_of_h0 from h0 and h1 from zz_h1;
# with it no group has members on both sides — the cross-label twin h2 / h2_as_rust included, which the per-label
# rule does not hold together (both are training files at this seed).
SEED = 1


def _pattern(seed):
    from PIL import Image
    coarse = np.random.RandomState(seed).randint(0, 256, (6, 6, 3)).astype(np.uint8)
    return Image.fromarray(coarse).resize((SIZE, SIZE), Image.BICUBIC)


def build_tree(root: Path) -> Path:
    from PIL import Image
    for cls, tag, base in (("healthy", "h", 0), ("rust", "r", 100)):
        d = root / "Apple" / cls
        d.mkdir(parents=True)
        for i in range(10):
            _pattern(base + i).save(d / f"{tag}{i}.jpg", quality=95)
    h, r = root / "Apple" / "healthy", root / "Apple" / "rust"
    shutil.copyfile(h / "h0.jpg", h / "copy_of_h0.jpg")
    shutil.copyfile(h / "h1.jpg", h / "zz_h1.jpg")
    shutil.copyfile(h / "h2.jpg", r / "h2_as_rust.jpg")
    for d, stem in ((h, "h3"), (h, "h4"), (r, "r3")):
        with Image.open(d / f"{stem}.jpg") as im:
            im.transpose(Image.FLIP_LEFT_RIGHT).save(d / f"{stem}_aug_flip_1.jpg", quality=90)
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory, cuda):
    from leaffliction_amd.cli.split import scan_dataset
    root = build_tree(tmp_path_factory.mktemp("dups") / "images")
    images = scan_dataset(root)
    assert len(images) == 26
    return root, images


@pytest.fixture(scope="module")
def decoded(tree):
    """The very tensors DeviceDecoder.chunks yields for the tree's files, on the host, and their reference hashes."""
    from leaffliction_amd.dataio.device_decode import DeviceDecoder
    _root, images = tree
    dec = DeviceDecoder()
    try:
        parts = [(kept, x.cpu().numpy()) for _f, kept, x, _n, _e in dec.chunks([str(im.src) for im in images], SIZE)]
    finally:
        dec.close()
    kept = [k for ks, _x in parts for k in ks]
    assert kept == list(range(len(images)))
    x = np.concatenate([x for _k, x in parts])
    sig = R.dhash128(x, 2)
    sig.setflags(write=False)
    return x, sig


def _index(images):
    return {im.rel_id.split("/")[-1][:-4]: k for k, im in enumerate(images)}


def test_find_duplicates_equals_reference_on_the_decoded_tensors(tree, decoded):
    from leaffliction_amd import nn
    from leaffliction_amd.dataio import duplicates as D
    _root, images = tree
    x, sig = decoded
    paths = [str(im.src) for im in images]
    assert np.array_equal(nn.dhash128(torch.from_numpy(x).cuda(), 2).cpu().numpy(), sig)
    for by, keys in ((("name", "hash"), D.name_keys(paths)), (("hash",), None)):
        found = D.find_duplicates(paths, threshold=T, img_size=SIZE, variants=2, by=by)
        want = R.hamming_pairs(sig, T)
        assert found.failed == [] and np.array_equal(found.pairs, want)
        assert found.groups == R.group(len(paths), want, keys)
    sigs, kept, errors = D.signatures(paths, img_size=SIZE, variants=8)
    assert kept == list(range(len(paths))) and errors == [] and tuple(sigs.shape) == (len(paths), 8, 4)
    assert np.array_equal(sigs.cpu().numpy(), R.dhash128(x, 8))


def test_byte_identical_copies_are_grouped_at_threshold_0(tree):
    from leaffliction_amd.dataio import duplicates as D
    _root, images = tree
    at = _index(images)
    found = D.find_duplicates([str(im.src) for im in images], threshold=0, img_size=SIZE, by="hash")
    rows = found.pairs.tolist()
    for a, b in (("copy_of_h0", "h0"), ("h1", "zz_h1"), ("h2", "h2_as_rust")):
        i, j = sorted((at[a], at[b]))
        assert [i, j, 0, 0] in rows
        assert any(i in g and j in g for g in found.groups)
    assert all(r[2] == 0 for r in rows)


def _write_manifest(path: Path, images, val):
    items = [{"plant": im.plant, "class": im.cls, "label": im.label,
              "split": "val" if im.rel_id.split("/")[-1][:-4] in val else "train", "src": im.src.as_posix(),
              "id": im.rel_id} for im in images]
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps({"meta": {}, "items": items}))
    return path


def _report(manifest: Path, out: Path, *extra, size=SIZE):
    from leaffliction_amd.cli import duplicates as C
    C.main(["--manifest", str(manifest), "--img-size", str(size), "--out", str(out), *extra])
    return json.loads((out / "duplicates.json").read_text())


def test_cli_reports_the_planted_cross_split_and_cross_label_groups(tree, tmp_path):
    _root, images = tree
    # copy_of_h0 in val, h0 in train; h1 and zz_h1 both in train; h2 in train, its copy under rust in val; r5 alone
    man = _write_manifest(tmp_path / "m.json", images, val={"copy_of_h0", "h2_as_rust", "r5", "h3", "h3_aug_flip_1"})
    doc = _report(man, tmp_path / "hash", "--by", "hash", "--threshold", "0")
    assert doc["meta"] == {"by": "hash", "threshold": 0, "variants": 2, "img_size": SIZE, "files": 26, "failed": 0}
    s = doc["summary"]
    assert s["cross_split_groups"] == 2 and s["val_files_with_train_duplicate"] == 2
    assert s["cross_label_groups"] == 1 and s["groups"] >= 3
    ids = [sorted(m["id"] for m in g["members"]) for g in doc["groups"]]
    assert ["Apple/healthy/h2.jpg", "Apple/rust/h2_as_rust.jpg"] in ids
    crossing = [g for g in doc["groups"] if g["splits"] == ["train", "val"]]
    assert len(crossing) == 2 and all(g["max_distance"] == 0 for g in crossing)
    lines = (tmp_path / "hash" / "duplicate_pairs.csv").read_text().splitlines()
    assert lines[0] == "a,b,distance,variant" and "Apple/healthy/copy_of_h0.jpg,Apple/healthy/h0.jpg,0,0" in lines
    # both rules: the balancer-named mirrors join, on one side of this manifest or the other
    both = _report(man, tmp_path / "both", "--by", "both", "--threshold", "0")
    assert both["summary"]["cross_split_groups"] == 2 and both["summary"]["groups"] >= 6
    # a directory scan knows no split
    from leaffliction_amd.cli import duplicates as C
    C.main(["--src", str(tree[0]), "--img-size", str(SIZE), "--out", str(tmp_path / "src"), "--threshold", "0"])
    scanned = json.loads((tmp_path / "src" / "duplicates.json").read_text())
    assert "cross_split_groups" not in scanned["summary"] and scanned["summary"]["cross_label_groups"] == 1
    assert all("split" not in m for g in scanned["groups"] for m in g["members"])


def test_split_group_duplicates_leaves_no_group_on_both_sides(tree, tmp_path):
    """(`split` hashes at 224 x 224, so the manifests are judged at that size too.)"""
    from leaffliction_amd.cli import split as S
    root, _images = tree
    plain, grouped = tmp_path / "plain", tmp_path / "grouped"
    S.main(["--src", str(root), "--out", str(plain), "--out-manifest", str(plain / "m.json"), "--seed", str(SEED)])
    S.main(["--src", str(root), "--out", str(grouped), "--out-manifest", str(grouped / "m.json"), "--seed", str(SEED),
            "--group-duplicates", "--group-by", "both", "--dup-threshold", "0"])
    doc = json.loads((grouped / "m.json").read_text())
    meta, side = doc["meta"], {it["id"]: it["split"] for it in doc["items"]}
    assert meta["grouped_by"] == "both" and meta["dup_threshold"] == 0
    after = _report(grouped / "m.json", tmp_path / "after", "--by", "both", "--threshold", "0", size=224)
    # what the flag promises whatever the seed: no group of ONE label has members on both sides
    one_label = [g for g in after["groups"] if len(g["labels"]) == 1]
    assert len(one_label) >= 5 and all(len(g["splits"]) == 1 for g in one_label)
    # what this seed adds, pinned on its own: the cross-label twin, which the per-label rule does not hold together,
    # has both its files in train
    assert side["Apple/healthy/h2.jpg"] == "train" and side["Apple/rust/h2_as_rust.jpg"] == "train"
    # and so the whole report is clean
    assert after["summary"]["cross_split_groups"] == 0 and after["summary"]["val_files_with_train_duplicate"] == 0
    before = _report(plain / "m.json", tmp_path / "before", "--by", "both", "--threshold", "0", size=224)
    assert before["summary"]["cross_split_groups"] >= 1
