"""cli/Transformation.py without a GPU: type names, output names, the image-number rule and the default output
directory, the folder walk, the skip / overwrite rule and argument errors (srcs/cli/Transformation.py)."""
import logging
from pathlib import Path

import pytest

from leaffliction_amd.cli import Transformation as T


def test_types_canonicalised_and_deduplicated(caplog):
    assert T.build_types_filter("mask, ROI,analyse,spots") == ("Mask", "ROI", "Analyze", "Brown")
    assert T.build_types_filter("Histogram,hist,HIST,disease,brown") == ("Hist", "Brown")
    assert T.build_types_filter("pseudo-landmarks,pseudolandmarks,landmarks,blur") == ("Landmarks", "Blur")
    with caplog.at_level(logging.WARNING):
        assert T.build_types_filter("mask,sharpen") == ("Mask",)
    assert "sharpen" in caplog.text
    assert T.build_types_filter("bogus") == T.DEFAULT_TYPES
    assert T.build_types_filter("") == T.DEFAULT_TYPES
    assert T.build_types_filter(None) == T.DEFAULT_TYPES
    assert T.build_types_filter(" , ,") == T.DEFAULT_TYPES
    assert T.DEFAULT_TYPES == ("Blur", "Mask", "ROI", "Analyze", "Landmarks", "Hist", "Brown")


def test_output_names():
    names = T.output_names("image (12)")
    assert names == {t: f"image (12)__T_{t}.jpg" for t in ("Blur", "Mask", "ROI", "Analyze", "Landmarks", "Hist",
                                                           "Brown")}


def test_image_number_and_default_out_dir():
    assert T.image_number("image (100)") == "100"
    assert T.image_number("Apple_healthy image (7) copy") == "7"
    assert T.image_number("image(3)") == "image(3)"
    assert T.image_number("leaf") == "leaf"
    root = Path(T.__file__).resolve().parents[2]
    assert T.default_out_dir(Path("/x/y/image (5).JPG")) == root / "artifacts" / "transformations" / "5"
    assert T.default_out_dir(Path("leaf.jpg")) == root / "artifacts" / "transformations" / "leaf"


def test_folder_walk(tmp_path):
    for rel in ("b/x.jpg", "a/deep/y.JPG", "a/z.png", "c.jpeg", "top.Jpg", "a/notes.txt", "d.jpg/inner.jpg"):
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    got = [p.relative_to(tmp_path).as_posix() for p in T.iter_images_in_dir(tmp_path)]
    assert got == ["a/deep/y.JPG", "b/x.jpg", "d.jpg/inner.jpg", "top.Jpg"]
    assert not T.is_image(tmp_path / "d.jpg")        # a directory named .jpg is no image
    assert not T.is_image(tmp_path / "missing.jpg")


def test_skip_and_overwrite_rule(tmp_path):
    new, old = tmp_path / "new.jpg", tmp_path / "old.jpg"
    old.write_bytes(b"x")
    assert T.should_write(new, False, False) and T.should_write(old, False, False)
    assert T.should_write(new, True, False) and not T.should_write(old, True, False)
    assert T.should_write(old, True, True) and T.should_write(old, False, True)


@pytest.mark.parametrize("argv,needle", [
    ([], "Must specify either single image"),
    (["-src", "{tmp}/nowhere", "-dst", "{tmp}/out"], "Source directory does not exist"),
    (["{tmp}/leaf.png"], "Not a valid image"),
    (["{tmp}/absent.jpg"], "Not a valid image"),
    (["-src", "{tmp}"], "Must specify either single image"),
    (["--config", "{tmp}/none.yaml", "{tmp}/leaf.png"], "Configuration file not found"),
])
def test_argument_errors_return_without_traceback(tmp_path, caplog, argv, needle):
    (tmp_path / "leaf.png").write_bytes(b"")
    argv = [a.replace("{tmp}", str(tmp_path)) for a in argv]
    with caplog.at_level(logging.ERROR):
        assert T.main(argv) is None
    assert needle in caplog.text
    assert not (tmp_path / "out").exists()


def test_empty_source_warns(tmp_path, caplog):
    (tmp_path / "src").mkdir()
    with caplog.at_level(logging.WARNING):
        T.main(["-src", str(tmp_path / "src"), "-dst", str(tmp_path / "dst")])
    assert "No images found" in caplog.text


def test_flags_match_the_reference():
    a = T.parse_args(["img.jpg", "--out-dir", "o", "--types", "mask", "--workers", "3", "--skip-existing",
                      "--overwrite", "--preview", "--config", "c.yaml"])
    assert (a.image, a.out_dir, a.types, a.workers, a.skip_existing, a.overwrite, a.preview, a.config) == \
        ("img.jpg", "o", "mask", 3, True, True, True, "c.yaml")
    b = T.parse_args(["-src", "s", "-dst", "d"])
    assert (b.src, b.dst, b.image, b.workers) == ("s", "d", None, 0)
    assert T.parse_args(["--src", "s", "--dst", "d"]).src == "s"
