/* Pure C11 consumer of the in-place graph edits of include/qv.h (qv_graph_remove, qv_graph_export_lists), the way a cgo
 * preamble sees them; links against libqv.so alone.  Without a GPU the index cannot be created (QV_ERR_NO_DEVICE) and only the
 * null-argument answers are checked.
 *   gcc -std=c11 -Wall -Werror -I include tests/c/graph_remove_smoke.c -L quiver_amd/lib -lqv -lm -Wl,-rpath,$PWD/quiver_amd/lib -o graph_remove_smoke */
#include "qv.h"
#include <stdio.h>
#include <string.h>
#include <math.h>

int main(void) {
    const uint32_t one = 0; uint32_t deg1 = 0, links1[64]; const int lv0 = 0;
    if (qv_graph_remove(NULL, &one, 1) != QV_ERR_INVALID_ARG || !strstr(qv_last_error(), "graph is null")) { fprintf(stderr, "remove(NULL): %s\n", qv_last_error()); return 2; }
    if (qv_graph_export_lists(NULL, &one, &lv0, 1, &deg1, links1) != QV_ERR_INVALID_ARG || !strstr(qv_last_error(), "graph is null")) { fprintf(stderr, "export_lists(NULL): %s\n", qv_last_error()); return 3; }
    if (qv_device_count() <= 0) { printf("no device: null-argument answers only\n"); return 0; }

    /* 200 points on a circle: a node's nearest neighbours are its angular neighbours */
    enum { N = 200, D = 4, M0 = 16 };
    static float pts[N][D]; static int8_t levels[N];
    for (int i = 0; i < N; i++) { double a = 6.283185307179586 * i / N; pts[i][0] = (float)cos(a); pts[i][1] = (float)sin(a); pts[i][2] = 0; pts[i][3] = 0; levels[i] = 0; }
    qv_index* gi = NULL; qv_graph* g = NULL; uint32_t first = 0;
    if (qv_index_create(&gi, D, QV_L2, 0, QV_FLAG_ROWMAJOR) != QV_OK || qv_index_add(gi, &pts[0][0], N, &first) != QV_OK) { fprintf(stderr, "graph index: %s\n", qv_last_error()); return 4; }
    if (qv_graph_build(&g, gi, N, levels, 8, M0, 50, 16, 4) != QV_OK) { fprintf(stderr, "graph build: %s\n", qv_last_error()); return 5; }
    uint32_t ep = 0; int lvl = -2;
    if (qv_graph_info(g, NULL, NULL, NULL, NULL, &ep, &lvl) != QV_OK) { fprintf(stderr, "graph info\n"); return 6; }
    /* delete node 50, the entry point and node 50 again (skipped); N is out of range and changes nothing */
    const uint32_t gone[3] = {50, ep, 50}, beyond[2] = {51, N};
    if (qv_graph_remove(g, beyond, 2) != QV_ERR_OUT_OF_RANGE) { fprintf(stderr, "a node >= n_nodes must be refused\n"); return 7; }
    if (qv_graph_remove(g, gone, 3) != QV_OK || qv_graph_remove(g, gone, 0) != QV_OK) { fprintf(stderr, "graph remove: %s\n", qv_last_error()); return 8; }
    if (qv_index_remove(gi, gone, ep == 50 ? 1 : 2) != QV_OK) { fprintf(stderr, "index remove: %s\n", qv_last_error()); return 9; }
    uint32_t ep2 = 0;
    if (qv_graph_info(g, NULL, NULL, NULL, NULL, &ep2, &lvl) != QV_OK || ep2 == ep || ep2 == 50 || lvl != 0) { fprintf(stderr, "entry point after remove: %u (was %u), level %d\n", ep2, ep, lvl); return 10; }
    /* the neighbours of 50 no longer list it, 50 itself answers degree 0, and 51 is still there */
    const uint32_t ask[3] = {49, 50, 51}; const int at[3] = {0, 0, 0}; uint32_t deg[3], links[3][M0];
    if (qv_graph_export_lists(g, ask, at, 3, deg, &links[0][0]) != QV_OK) { fprintf(stderr, "export lists: %s\n", qv_last_error()); return 11; }
    if (deg[1] != 0 || (ep != 49 && deg[0] == 0) || (ep != 51 && deg[2] == 0)) { fprintf(stderr, "degrees %u %u %u\n", deg[0], deg[1], deg[2]); return 12; }
    for (int j = 0; j < 3; j += 2) for (uint32_t t = 0; t < deg[j]; t++) if (links[j][t] == 50) { fprintf(stderr, "node %u still lists 50\n", ask[j]); return 13; }
    /* a search for node 50's vector finds its live angular neighbours */
    const float gq[D] = {pts[50][0], pts[50][1], 0, 0};
    uint32_t gr[2], gc = 0; float gd[2];
    if (qv_graph_search(g, gq, 1, 2, 32, gr, gd, &gc, NULL) != QV_OK || gc != 2) { fprintf(stderr, "graph search: %s\n", qv_last_error()); return 14; }
    if (gr[0] == 50 || gr[1] == 50 || gr[0] == ep || gr[1] == ep || !(gd[0] > 0.0f)) { fprintf(stderr, "graph result [%u %u]\n", gr[0], gr[1]); return 15; }
    qv_graph_destroy(g); qv_index_destroy(gi);
    printf("ok: entry %u -> %u, search [%u %u]\n", ep, ep2, gr[0], gr[1]);
    return 0;
}
