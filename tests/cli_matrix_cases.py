"""The cases of tests/test_cli_matrix.py and tests/golden/make_cli_matrix.py: `igd search db.igd <base> <x> <y>` for every
base and every ORDERED pair of tokens, in a directory that holds nothing but the files below under relative names (so that no
transcript carries a path).  One definition for the recorder and the replay: the fixture keeps one outcome per case in the
order cases() yields them."""
import hashlib
import os
import shutil
import subprocess

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# a token that is a bare letter is that option with its value missing
TOKENS = [t.split() for t in """
-f | -m | -s | -c | -u | -b | -w | -X | -C | -G | -E | -R | -J
-q q.bed | -r chr1 1 100000 | -v 500 | -Q list | -U u.bed | -P 5 | -P 0 | -g genome | -S 3
-M circular | -M shuffle | -M resample | -M bogus | -O 5 | -A 0.5 | -B 2
-N 100 | -N -5 | -H -5,0,5 | -H 5,0 | -L 10 | -L | -V sum | -V median
-D 100 | -D -1 | -W ws.bed | -K groups | -Z 100,10 | -Z x | -o hm
-q | -U | -P | -N | -H | -V | -D | -W | -K | -Z | -g | -S | -M | -O
""".replace("\n", " | ").split(" | ") if t.strip()]
BASES = [[], ["-q", "q.bed"], ["-q", "q.bed", "-P", "5", "-g", "genome"], ["-Q", "list", "-N", "50"]]
ENV = {"IGD_HOST_MAX_QUERIES": "100000000"}
NEEDS_ENGINE = 69                      # exit code of an accepted command that only the engine computes, where there is no GPU


def cases():
    for base in BASES:
        for x in TOKENS:
            for y in TOKENS:
                yield base + x + y


def make_workdir(d):
    for f in ("db.igd", "db_index.tsv", "q.bed"):
        shutil.copy(os.path.join(GOLDEN, "branch", f), os.path.join(d, f))
    head = open(os.path.join(d, "q.bed")).readlines()[:50]
    for f in ("u.bed", "ws.bed"):
        open(os.path.join(d, f), "w").writelines(head)
    with open(os.path.join(d, "genome"), "w") as g:
        g.writelines("chr%s\t300000000\n" % c for c in [*range(1, 23), "X", "Y"])
    open(os.path.join(d, "list"), "w").write("q.bed\nq.bed\n")
    open(os.path.join(d, "groups"), "w").close()


def run(igd, d, args):
    """(exit code, 16 hex digits of sha256(stdout), the same of stderr, first line of the stream that spoke)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("IGD_")}
    p = subprocess.run([igd, "search", "db.igd", *args], cwd=d, env=dict(env, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    spoke = (p.stdout or p.stderr).decode(errors="replace").splitlines()
    return [p.returncode, hashlib.sha256(p.stdout).hexdigest()[:16], hashlib.sha256(p.stderr).hexdigest()[:16], spoke[0] if spoke else ""]
