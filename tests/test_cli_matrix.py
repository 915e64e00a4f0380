"""`igd search` answers every case of tests/cli_matrix_cases.py -- 4 bases x 58 x 58 ordered pairs of option tokens -- exactly
as tests/golden/cli_matrix.json recorded it from the commit before the command line became one option table and one ordered
list of refusals: exit code, stdout and stderr.  The other *_cli tests pin chosen refusals; this one pins which refusal answers
when two apply, and what a value looked at again as an option does."""
import json
import os
import shutil
from concurrent.futures import ThreadPoolExecutor

import cli_matrix_cases as M
from helpers import ROOT, short_tmpdir

IGD = os.path.join(ROOT, "bin", "igd")


def test_every_pair_of_options_answers_as_recorded():
    fx = json.load(open(os.path.join(M.GOLDEN, "cli_matrix.json")))
    cases = list(M.cases())
    assert len(cases) == len(fx["case"]) == 4 * 58 * 58
    # accepted commands that only the engine computes are left out (no GPU work in an unmarked test); they stay few
    skip = set(fx["needs_engine"])
    assert len(skip) <= len(cases) // 100
    d = short_tmpdir("igcm")
    try:
        M.make_workdir(d)
        todo = [i for i in range(len(cases)) if i not in skip]
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
            got = list(pool.map(lambda i: M.run(IGD, d, cases[i]), todo))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    bad = [(cases[i], fx["outcomes"][fx["case"][i]], g) for i, g in zip(todo, got) if g[:3] != fx["outcomes"][fx["case"][i]][:3]]
    assert not bad, "%d of %d cases differ; (arguments, recorded, got): %s" % (len(bad), len(todo), bad[:5])
