"""`python -m leaffliction_amd.cli.convert_model SRC DST [--to keras|npz]`: rewrite a leaf_cnn
archive in the other layout.  SRC may be this package's npz archive or a Keras 3 `.keras`
archive; it is read by `load_model` and written by `LeafCNN.save(DST, format=...)`, so the
weights go through the model unchanged (the model lives on the GPU: there is no CPU path)."""
from __future__ import annotations

import argparse
import sys

from ..utils.common import get_logger, setup_logging

logger = get_logger(__name__)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Convert a leaf_cnn .keras archive between the npz and Keras layouts")
    p.add_argument("src", help="archive to read (npz or Keras layout)")
    p.add_argument("dst", help="archive to write")
    p.add_argument("--to", choices=["keras", "npz"], default="keras", help="layout of DST (default: keras)")
    return p.parse_args(argv)


def main(argv=None) -> int:
    setup_logging()
    args = parse_args(argv)
    from ..model.cnn import load_model
    try:
        model = load_model(args.src)
        model.save(args.dst, format=args.to)
    except (ValueError, OSError) as e:
        logger.error("%s", e)
        return 1
    logger.info("%s -> %s (%s layout)", args.src, args.dst, args.to)
    return 0


if __name__ == "__main__":
    sys.exit(main())
