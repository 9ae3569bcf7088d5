#!/usr/bin/env python3
"""Drop-in for the reference's py/freddie_segment_vis.py: same command line, same files in, same pickle out.
The per-object coverage classes run on the GPU (freddie_amd/segment_vis.py, include/freddie_vis.h); see INTEGRATION.md."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from freddie_amd.segment_vis import main  # noqa: E402

if __name__ == "__main__":
    main()
