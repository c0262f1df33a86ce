"""sslap_amd -- MI355X-native auction solver for sparse linear assignment problems.

Drop-in for the hot path of OllieBoyne/sslap: `auction_solve`, `from_matrix` / `from_sparse`
(the reference's `_from_matrix` / `_from_sparse`), `AuctionSolver` and the feasibility guard `hopcroft_solve`, plus
`auction_solve_batch` / `auction_solve_sparse_batch` / `auction_solve_ell_batch` (many small dense / sparse problems in
one launch, one workgroup each; the last from padded candidate lists (B, N, K); the three take `outside=` for partial assignments),
`auction_solve_points_batch` (the dense batch from two point sets, costs |x_i - y_j|^2 formed from the coordinates; with
`candidates=K` through candidate lists that `points_candidates` builds on the device), `auction_solve_boxes_batch` (the
same from two box sets, costs 1 - IoU or 1 - GIoU; `boxes_candidates` builds its lists) and `hopcroft_solve_batch` (the matching of many small graphs in one launch).  Everything computes on the GPU
through libmisslap.so (hand-written HIP for gfx950, C ABI in include/misslap.h); importing the
package never touches the GPU, but every solver call raises if the library or the GPU is missing.
"""
from .auction_solve import AuctionSolver, auction_solve, from_matrix, from_sparse, _from_matrix, _from_sparse
from .check_feasible import hopcroft_solve
from .dense_batch import (auction_solve_batch, batch_meta_to_host, dense_reverse_finish, dense_to_augmented, dense_to_packed,
                          raise_for_status)
from .sparse_batch import auction_solve_sparse_batch, sparse_reverse_finish, sparse_to_augmented
from .ell_batch import auction_solve_ell_batch, ell_to_packed
from .matching_batch import hopcroft_solve_batch
from .points_batch import (auction_solve_points_batch, points_candidates, points_reverse_finish, points_to_dense,
                           points_to_ell)
from .boxes_batch import auction_solve_boxes_batch, boxes_candidates, boxes_to_dense, boxes_to_ell

__version__ = "0.1.0"
solve_batch = AuctionSolver.solve_batch  # many problems with the same number of persons in lockstep on one GPU (include/misslap.h: misslap_solve_batch)
__all__ = ["auction_solve", "auction_solve_batch", "auction_solve_sparse_batch", "auction_solve_ell_batch", "auction_solve_points_batch", "points_to_dense", "points_reverse_finish", "points_to_ell", "points_candidates", "auction_solve_boxes_batch", "boxes_to_dense", "boxes_to_ell", "boxes_candidates", "ell_to_packed", "dense_to_augmented", "dense_to_packed", "dense_reverse_finish", "sparse_to_augmented", "sparse_reverse_finish", "batch_meta_to_host", "raise_for_status", "hopcroft_solve", "hopcroft_solve_batch", "from_matrix", "from_sparse", "AuctionSolver", "solve_batch"]
