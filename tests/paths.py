"""Where the tests find things: the repository, the fixtures, and the reference library that oracle/Makefile's `ref` target builds
where the reference's sources exist (the live tests skip without it)."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libx264ref.so")
