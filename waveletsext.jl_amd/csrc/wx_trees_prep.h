// wx_trees_prep.h -- a matrix of per-signal trees that lives in DEVICE memory (what wx_treeselect_batch_* writes), prepared for its
// consumers without a trip to the host: wx_trees_prep.hip.
#pragma once
#include "wx_common.h"

// which way the last per-signal-tree call of this thread went (wx_wpt_trees_last_route, include/waveletsext_hip.h)
enum {
    WX_TREES_ROUTE_NONE = 0,      // no such call yet, or the last one returned an error before it chose
    WX_TREES_ROUTE_HOST = 1,      // trees in host memory
    WX_TREES_ROUTE_DEV_LDS = 2,   // device trees: prep kernel, its bits and depths feed k_wpt_trees
    WX_TREES_ROUTE_DEV_SINGLE = 3,// device trees, all columns equal: prep kernel, column 0 to the host, the single-tree entry
    WX_TREES_ROUTE_DEV_COPIED = 4,// device trees outside the LDS kernel's window: the matrix copied to the host, then as HOST
    WX_TREES_ROUTE_DEV_GATHER = 5 // device trees: prep kernel, the gather reads the caller's matrix
};
void wx_trees_route_set(int route);

// One launch over the (ntree, batch) byte matrix `trees` (device memory of the current device, any non-zero byte = decomposed;
// quad = false: binary heap, children 2i and 2i + 1; quad = true: children 4i - 2 .. 4i + 1) and ONE wait for the stream:
//   every column is a valid tree, else WX_EASSERT; k > 0: every depth < k, else WX_EARG; the lowest offending column decides;
//   bits   != nullptr: the columns in the layout of wx_tree_bits.h (node i is bit i - 1, either heap), nw words each, every word written;
//   depths != nullptr: one byte per column, the depth of the deepest decomposed node + 1 (0 for the bare root);
//   same   != nullptr: whether every column equals column 0 byte for byte, and col0 (ntree bytes, host) receives that column.
// Returns WX_OK, the two codes above (message set) or WX_EHIP.  ntree == 0: nothing to check, *same = true.
int wx_trees_prep(bool quad, const uint8_t *trees, int64_t ntree, int64_t batch, int k, uint32_t *bits, int nw, uint8_t *depths,
                  uint8_t *col0, bool *same, hipStream_t st);

// The same for a matrix in HOST memory, in one pass over its columns (wx_isvalidtree*, wx_tree_depth*; m = the signal length or
// the image's rows, n = its columns, read for quad trees only); a matrix of 2^22 bytes and more is shared by up to 8 threads, a
// contiguous range of columns each.  max_depth >= 0: no tree is deeper than it, else WX_EASSERT with the message of the sides
// (images pass the levels both sides divide by); as above, the lowest offending column decides, and it is counted once: as
// invalid, else as deeper than the sides, else as too deep for k.  `bits` is zero on entry and written for the columns that passed;
// `same` needs no col0, the caller has the matrix.  Needs no device.
int wx_trees_check_host(bool quad, int64_t m, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, int k, int max_depth,
                        uint32_t *bits, int nw, uint8_t *depths, bool *same);
