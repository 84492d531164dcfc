"""tests/golden/make_c1_launch_golden.py as a module (`rec`) and the golden it wrote (`GOLDEN`), for the two tests that read them"""
import importlib.util
import json
import os

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_c1_launch_golden.py")
_spec = importlib.util.spec_from_file_location("make_c1_launch_golden", _PATH)
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)
with open(rec.GOLDEN) as f:
    GOLDEN = json.load(f)
