"""Test fixture locations."""
import os

VENDORED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref")


def ref_path(rel: str) -> str:
    """A reference golden file: the vendored copy under tests/fixtures/ref (see tools/vendor_fixtures.py).  The
    tests read nothing outside the repository."""
    return os.path.join(VENDORED, rel)
