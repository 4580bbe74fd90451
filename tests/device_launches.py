"""The launch scaffolding of the GPU suites: Launches, renderer_render, assert_same, SAME, SQUARE, counter_names,
omp_threads, planar_states, run, gpu_run.  All of it is tools/gpu_launches.py, which tools/gpu_fuzz.py uses too; the suites
import it under this name."""

import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from gpu_launches import *  # noqa: E402,F401,F403
