#!/usr/bin/env python3
"""Drop-in for the reference's py/freddie_cluster.py: segment_*.tsv in, cluster_*.tsv out, the same flags and directory layout.
The rounds' models are built on the GPU, the solve is HiGHS (freddie_amd/cluster.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from freddie_amd import cluster  # noqa: E402

if __name__ == "__main__":
    sys.exit(cluster.main())
