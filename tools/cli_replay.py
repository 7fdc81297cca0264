#!/usr/bin/env python3
"""Output identity of the command line between two checkouts, on the stub databases of the CLI tests:

    python tools/cli_replay.py BEFORE_CHECKOUT AFTER_CHECKOUT

In each checkout (both built) the host-only CLI test modules are run with cli.run and cli._run_on wrapped: every call is
recorded with its options, exit code or exception, the text written to `out`, and every method call and attribute write the
database object received, arguments included.  The two recordings must be equal, call for call; the times printed and the
temporary database paths are masked.  Exit status 0: identical."""
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

MODULES = ("tests/test_*_cli.py", "tests/test_api_mirror.py", "tests/test_time_buckets_host.py", "tests/test_time_group_host.py",
           "tests/test_wide_group_host.py", "tests/test_group_error_host.py", "tests/test_grouped_distinct_host.py")


def _mask(text):
    return re.sub(r"0x[0-9a-fA-F]+", "0x?", re.sub(r"execution time: [0-9.]+ ms", "execution time: ? ms", text))


class _Recorded:
    """Stands for the database object: forwards everything, keeps what it was asked."""

    def __init__(self, db, calls):
        object.__setattr__(self, "_db", db)
        object.__setattr__(self, "_calls", calls)

    def __getattr__(self, name):
        value = getattr(self._db, name)
        if not callable(value):
            return value

        def call(*args, **kwargs):
            self._calls.append([name, _mask(repr(args)), {k: _mask(repr(v)) for k, v in sorted(kwargs.items())}])
            return value(*args, **kwargs)
        return call

    def __setattr__(self, name, value):
        self._calls.append(["set " + name, repr(value), {}])
        setattr(self._db, name, value)


def record(path):
    """Run the modules here, in this checkout, and write what the wrapped entry points saw."""
    sys.path.insert(0, os.getcwd())
    import pytest
    from approximatequeryengine_amd import cli
    assert os.path.dirname(os.path.dirname(os.path.abspath(cli.__file__))) == os.getcwd(), cli.__file__
    seen = []

    def wrapped(name, original, db_at):
        def entry(*args, **kwargs):
            ns = args[db_at + 1] if db_at is not None else args[0]
            out = args[db_at + 2] if db_at is not None else (args[1] if len(args) > 1 else kwargs.get("out"))
            entry_ = {"entry": name, "options": {k: repr(v) for k, v in sorted(vars(ns).items()) if k != "db"}, "calls": []}
            if db_at is not None:
                args = args[:db_at] + (_Recorded(args[db_at], entry_["calls"]),) + args[db_at + 1:]
            seen.append(entry_)  # (in call order: run before the _run_on it reaches)
            try:
                entry_["status"] = original(*args, **kwargs)
                return entry_["status"]
            except BaseException as e:
                entry_["raised"] = _mask(repr(e))
                raise
            finally:
                text = out.getvalue() if hasattr(out, "getvalue") else ""
                entry_["out"] = _mask(text.replace(str(ns.db), "<db>"))
        return entry

    cli.run = wrapped("run", cli.run, None)
    cli._run_on = wrapped("_run_on", cli._run_on, 0)
    modules = sorted(m for pattern in MODULES for m in glob.glob(pattern))
    status = pytest.main(["-q", "-p", "no:cacheprovider", "-m", "not gpu", *modules])
    with open(path, "w") as f:
        json.dump({"pytest": int(status), "seen": seen}, f)


def main(argv):
    if len(argv) == 2 and argv[0] == "--record":
        return record(argv[1])
    if len(argv) != 2:
        print(__doc__)
        return 2
    got = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, checkout in enumerate(argv):
            path = os.path.join(tmp, f"{i}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--record", path], cwd=checkout, check=True, stdout=subprocess.DEVNULL)
            with open(path) as f:
                got.append(json.load(f))
    before, after = got
    differing = [i for i, (a, b) in enumerate(zip(before["seen"], after["seen"])) if a != b]
    print(f"pytest status: {before['pytest']} / {after['pytest']}")
    print(f"entries recorded: {len(before['seen'])} / {len(after['seen'])} "
          f"(run: {sum(e['entry'] == 'run' for e in after['seen'])}, _run_on: {sum(e['entry'] == '_run_on' for e in after['seen'])}; "
          f"database calls: {sum(len(e['calls']) for e in after['seen'])})")
    print(f"entries that differ: {len(differing)}")
    for i in differing[:5]:
        print(json.dumps(before["seen"][i], indent=1), "\n  !=\n", json.dumps(after["seen"][i], indent=1))
    return 0 if not differing and len(before["seen"]) == len(after["seen"]) and before["pytest"] == after["pytest"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
