"""`split --group-duplicates` on the host: build_split_map with groups, the CLI with the name rule, and
`cli.duplicates --by name` without a GPU."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((ROOT / "tests" / "golden" / "split_golden.json").read_text())
SEED = 32   # the CLI's default; checked below to split at least one family of the tree when the flag is absent


def _golden_tree(root):
    for plant, classes in GOLD["layout"].items():
        for cls, n in classes.items():
            d = root / plant / cls
            d.mkdir(parents=True)
            for i in range(n):
                (d / f"image ({i + 1}).{'JPG' if i % 2 else 'jpg'}").write_bytes(b"")
    return root


def _by_label(images):
    out = {}
    for im in images:
        out.setdefault(im.label, []).append(im)
    return out


def test_no_groups_and_singleton_groups_reproduce_the_golden_maps(tmp_path):
    from leaffliction_amd.cli import split as S
    images = S.scan_dataset(_golden_tree(tmp_path / "images"))
    by_label = _by_label(images)
    singletons = {im.rel_id: k for k, im in enumerate(images)}
    for case in GOLD["cases"]:
        assert S.build_split_map(by_label, case["alloc"], case["seed"]) == case["split"]
        assert S.build_split_map(by_label, case["alloc"], case["seed"], None) == case["split"]
        assert S.build_split_map(by_label, case["alloc"], case["seed"], {}) == case["split"]
        assert S.build_split_map(by_label, case["alloc"], case["seed"], singletons) == case["split"]


def _planted():
    from leaffliction_amd.cli.split import SourceImage
    images, groups = [], {}

    def add(label, name, gid=None):
        rel = f"P/{label}/{name}.jpg"
        images.append(SourceImage("P", label, f"P__{label}", Path("/nowhere") / rel, rel))
        if gid is not None:
            groups[rel] = gid
    for i in range(20):                     # families of 1..4 files
        add("a", f"a{i}", gid=i // 4 if i < 12 else None)
    for i in range(6):                      # one label that is a single group
        add("whole", f"w{i}", gid=100)
    for i in range(9):                      # a group larger than the allocation, and loose files
        add("b", f"b{i}", gid=200 if i < 5 else None)
    add("single", "s0")
    return images, groups


@pytest.mark.parametrize("seed", [0, 1, 32, 12345])
def test_planted_groups_stay_on_one_side(seed):
    from leaffliction_amd.cli import split as S
    images, groups = _planted()
    by_label = _by_label(images)
    counts = {lab: len(v) for lab, v in by_label.items()}
    for alloc in (S.allocate_validation_by_ratio(counts, 0.2), S.allocate_validation_by_ratio(counts, 0.5),
                  S.allocate_validation_counts(counts, 100)):
        sm = S.build_split_map(by_label, alloc, seed, groups)
        assert sm == S.build_split_map(by_label, alloc, seed, dict(groups))          # deterministic per seed
        assert set(sm) == {im.rel_id for im in images} and set(sm.values()) <= {"train", "val"}
        sides = {}
        for rel, gid in groups.items():
            sides.setdefault(gid, set()).add(sm[rel])
        assert all(len(s) == 1 for s in sides.values()), sides                       # members share a side
        for lab, ims in by_label.items():
            n_val = sum(sm[im.rel_id] == "val" for im in ims)
            assert n_val <= alloc[lab] <= max(0, len(ims) - 1)
            assert n_val < len(ims)                                                  # a training image is left
        assert sides[100] == {"train"}                                               # the single-group label
        if alloc["P__b"] < 5:
            assert sides[200] == {"train"}
    assert S.build_split_map(by_label, alloc, 1, groups) != S.build_split_map(by_label, alloc, 2, groups)


def _family_tree(root):
    """Empty .jpg-named files: 2 labels, 10 originals each, 3 balancer-named copies of every second one."""
    for cls in ("healthy", "rust"):
        d = root / "Apple" / cls
        d.mkdir(parents=True)
        for i in range(10):
            (d / f"leaf_{i}.JPG").write_bytes(b"")
            if i % 2 == 0:
                for k, t in enumerate(("flip", "rotate", "crop")):
                    (d / f"leaf_{i}_aug_{t}_{k + 1}.JPG").write_bytes(b"")
    return root


def _families_on_both_sides(manifest):
    from leaffliction_amd.dataio.duplicates import family_key
    sides = {}
    for it in json.loads(Path(manifest).read_text())["items"]:
        sides.setdefault((it["label"], family_key(it["id"])), set()).add(it["split"])
    return sum(len(s) > 1 for s in sides.values())


def test_cli_group_by_name_keeps_families_together(tmp_path):
    from leaffliction_amd.cli import split as S
    root = _family_tree(tmp_path / "images")
    plain, grouped = tmp_path / "plain", tmp_path / "grouped"
    S.main(["--src", str(root), "--out", str(plain), "--out-manifest", str(plain / "m.json"), "--seed", str(SEED)])
    S.main(["--src", str(root), "--out", str(grouped), "--out-manifest", str(grouped / "m.json"), "--seed", str(SEED),
            "--group-duplicates", "--group-by", "name"])
    assert _families_on_both_sides(plain / "m.json") >= 1       # the leak the flag is for, at this seed
    assert _families_on_both_sides(grouped / "m.json") == 0
    meta_plain = json.loads((plain / "m.json").read_text())["meta"]
    meta = json.loads((grouped / "m.json").read_text())["meta"]
    assert "grouped_by" not in meta_plain and "dup_threshold" not in meta_plain
    assert meta["grouped_by"] == "name" and meta["dup_threshold"] is None     # no hash, so no threshold applied
    assert sorted(set(meta) - set(meta_plain)) == ["dup_threshold", "grouped_by"]
    items = json.loads((grouped / "m.json").read_text())["items"]
    for lab in ("Apple__healthy", "Apple__rust"):
        n_val = sum(it["split"] == "val" for it in items if it["label"] == lab)
        assert 1 <= n_val <= 5                                  # ratio 0.2 of 25 files allocates 5


def test_cli_duplicates_by_name_runs_without_a_gpu(tmp_path):
    root = _family_tree(tmp_path / "images")
    out = tmp_path / "dups"
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="",
               PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "leaffliction_amd.cli.duplicates", "--src", str(root), "--by", "name",
                          "--out", str(out)], env=env, cwd=tmp_path, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    doc = json.loads((out / "duplicates.json").read_text())
    assert doc["meta"]["files"] == 50 and doc["meta"]["failed"] == 0 and doc["meta"]["by"] == "name"
    assert doc["summary"] == {"groups": 10, "files_in_groups": 40, "cross_label_groups": 0}
    first = doc["groups"][0]
    assert [m["id"] for m in first["members"]] == [
        "Apple/healthy/leaf_0.JPG", "Apple/healthy/leaf_0_aug_crop_3.JPG", "Apple/healthy/leaf_0_aug_flip_1.JPG",
        "Apple/healthy/leaf_0_aug_rotate_2.JPG"]
    assert first["labels"] == ["Apple__healthy"] and first["max_distance"] is None and first["splits"] == []
    assert (out / "duplicate_pairs.csv").read_text().splitlines() == ["a,b,distance,variant"]
