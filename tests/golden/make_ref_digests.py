"""Writes tests/golden/oracle_vs_ref_digests.json: the UNMODIFIED reference's answer (oracle/_ref/yttm_ref_{det,prod}, built by
oracle/Makefile) to every case of tests/test_oracle_vs_ref.py, as the md5 of its model file or ids, or its error message.  The test
compares the oracle with these digests wherever it runs.  Needs the reference sources (make -C oracle ref):

    python tests/golden/make_ref_digests.py

Delete the JSON first to record it from scratch (an existing digest that the reference contradicts fails the run)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)


def main():
    rc = pytest.main([os.path.join(TESTS, "test_oracle_vs_ref.py"), "-q", "-p", "no:cacheprovider"])
    t = sys.modules["test_oracle_vs_ref"]
    if rc != 0 or not t.LIVE:
        raise SystemExit("not written: %s" % ("the tests failed" if rc != 0 else "oracle/_ref is not built"))
    with open(t.DIGESTS, "w") as f:
        json.dump(dict(sorted(t.RECORDED.items())), f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(t.RECORDED), os.path.relpath(t.DIGESTS, os.path.dirname(TESTS))))


if __name__ == "__main__":
    main()
