/* cli_san_main.c -- harness for tests/test_cli_leaks_host.py: igd_search() as a LIBRARY entry, called six times in one process --
 * refusals of every kind, an accepted command between them, the first refusal again -- so that what a refused call leaves
 * behind shows under the host sanitizers.  Compiled with igd_cli_abi.c, igd_core.c, igd_hostpath.c, igd_create.c and
 * igd_hip_lazy.c; needs no engine library as long as the host route takes the accepted command.
 * usage: cli_san <directory with db.igd, db_index.tsv, q.bed, genome and an empty groups>
 * Every call's stdout follows a line "== <n>"; the exit code is 0 when every call returned what it should. */
#include <stdio.h>
#include <sysexits.h>
#include <unistd.h>
#include "igd_search.h"

#define ARGS(...) {"igd", "search", "db.igd", __VA_ARGS__, NULL}
static const struct { int rc; char *argv[16]; } CALLS[] = {
    {EX_USAGE, ARGS("-q", "q.bed", "-H", "1,2")},                                        /* a newer refusal */
    {EX_OK, ARGS("-q", "q.bed", "-u", "-N", "5")},                                       /* an older one */
    {EX_USAGE, ARGS("-q", "q.bed", "-g", "genome", "-P", "3", "-Z", "100,10", "-u")},    /* -Z: its offsets are parsed by then */
    {EX_USAGE, ARGS("-q", "q.bed", "-u", "-K", "groups")},                               /* -K: the file names no group */
    {EX_OK, ARGS("-q", "q.bed", "-u")},
    {EX_USAGE, ARGS("-q", "q.bed", "-H", "1,2")},
};

int main(int argc, char **argv)
{
    if (argc < 2 || chdir(argv[1]) != 0) return 2;
    int bad = 0;
    for (int k = 0; k < (int)(sizeof CALLS / sizeof *CALLS); k++) {
        int n = 0;
        while (CALLS[k].argv[n]) n++;
        printf("== %d\n", k);
        const int rc = igd_search(n, (char **)CALLS[k].argv);
        fflush(stdout);
        if (rc != CALLS[k].rc) { fprintf(stderr, "call %d returned %d, not %d\n", k, rc, CALLS[k].rc); bad = 1; }
    }
    return bad;
}
