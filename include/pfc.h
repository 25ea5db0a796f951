/*
 * pfc.h — C ABI of libpfc_hip: the MI355X (gfx950) implementation of PressureFieldContact.jl's per-contact-pair
 * hot path (OBB-BVH culling -> tet/triangle clipping -> pressure + friction wrench integration).
 *
 * The reference (pure Julia) has no FFI for this path; its only substitution hook is the `de::Function` field of
 * MechanismScenario (src/mechanism_scenario.jl:175,181, invoked at src/radau/radau_functions.jl:9,67).  A
 * replacement `calcXd_hip!` is calcXd! (src/contact_algorithms_non_friction.jl:18-38) with
 * `forceAllElasticIntersections!` (:60-68) replaced by ONE call of pfc_eval() for all contact instructions; the
 * Julia `ccall` stubs are in INTEGRATION.md.  Each entry point below names the reference code it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - All indices crossing the ABI are 0-based (the Julia shim subtracts 1).
 *   - All matrices are column-major (Julia / StaticArrays order).
 *   - Host-pointer entry points copy in/out; the caller owns its buffers.  The library owns all device memory.
 *   - Every function returns a pfc_status (0 = ok, >0 = error) unless documented to return an id or a count
 *     (>= 0) in which case errors are returned as -(pfc_status).
 *   - A handle is not re-entrant (the reference scenario is not either: shared m.TT_Cache / tm.bodyBodyCache,
 *     src/contact_algorithms_non_friction.jl:95,120); different handles may be used from different threads.
 *   - The library never falls back to a CPU path: without a usable HIP device pfc_create() fails.
 */
#ifndef PFC_H
#define PFC_H

#ifdef __cplusplus
extern "C" {
#endif

#define PFC_VERSION 100
#define PFC_INTERNAL_NODE (-9999) /* leaf sentinel of internal nodes: src/obb/tree_types.jl:11,56 */

typedef enum {
    PFC_OK = 0,
    PFC_ERR_NONFINITE = 1, /* error("Non-finite vertex likely"): src/clip/static_clip.jl:52 ; singular tet */
    PFC_ERR_OVERFLOW = 2,  /* a device work list overflowed; capacities were grown, re-issue the evaluation */
    PFC_ERR_BAD_ARG = 3,   /* bad id / size / NULL pointer; "something is wrong": src/clip/static_clip.jl:13 */
    PFC_ERR_NOMEM = 4,
    PFC_ERR_HIP = 5,       /* HIP runtime failure, see pfc_last_error() */
    PFC_ERR_STATE = 6,     /* call order violated (e.g. add_mesh after finalize) */
    PFC_ERR_INVERTED_TET = 7 /* error("inverted tetrahedron"): src/geometry/mesh.jl:28 */
} pfc_status;

typedef enum { PFC_REGULARIZED = 0, PFC_BRISTLE = 1 } pfc_friction_model;

typedef struct pfc_context *pfc_handle;

/* Library/ABI version (PFC_VERSION of the build). */
int pfc_version(void);
/* 0 for the product build.  Diagnostic builds report themselves: bit 0 = in-kernel phase stamps (-DPFC_STAMPS, graph
 * replay off), bits 8..15 = elimination variant (-DPFC_EXP=n: one phase of the narrowphase compiled out, WRONG results),
 * bit 16 = an A/B variant built from patched sources (scripts/mkvar.sh, -DPFC_VARIANT).
 * The Python binding refuses to load a non-product build unless PFC_ALLOW_DIAGNOSTIC=1 is set. */
int pfc_build_info(void);

/* MechanismScenario() (src/mechanism_scenario.jl:181-198): creates an empty scenario bound to HIP device
 * `device`.  Fails with PFC_ERR_HIP when no device is usable. */
int pfc_create(int device, pfc_handle *out);
/*
 * The same scenario over SEVERAL devices of the node for the one host process the reference is (its calcXd! loops over the
 * contact instructions in a single Julia process, src/contact_algorithms_non_friction.jl:60-68; SURVEY section 8(b):
 * "pfc_create(device_mask)").  devices[0..n_devices) are HIP device ordinals (an ordinal may appear more than once: several
 * shard contexts on one device).  Every other entry point takes the handle unchanged:
 *   - pfc_add_mesh / pfc_add_instruction / pfc_finalize replicate meshes, trees and instructions on every device;
 *   - an evaluation cuts its items into contiguous ranges, one per device, balanced by cost (node tests + candidates of the
 *     previous evaluation of the same item list; the leaf-count product of the two meshes the first time), SURVEY 8(e).  Items
 *     are independent, there is no collective:
 *       host-pointer entry points (pfc_eval, pfc_eval_dual, pfc_eval_dual_bp): one library thread per device evaluates its
 *       range straight from / into the caller's arrays;
 *       device-pointer entry points (pfc_eval_device, pfc_eval_dual_device[_bp|_more], pfc_scatter_generalized_device): the
 *       buffers live on devices[0]; the other devices get their ranges by peer copies (xGMI) and write their results back the
 *       same way, ordered against `stream` by events; pfc_check synchronises every device.
 *   - option "multi_min" (default 8): with fewer than this many items per device fewer devices take part
 *     (pfc_last_shards() tells how many did); every other option is forwarded to all devices;
 *   - the partition rule (csrc/pfc_partition.h; tests/partition_reference.py states it a second time).  For n items on K devices:
 *       k_use = clamp(n / max(multi_min, 1), 1, K) devices take part, the others idle;
 *       cost of item i = 64 + 0.02 * leaves(mesh_1) * leaves(mesh_2) the first time an item list is evaluated (64 where the ids
 *       are device data the host cannot read), and 64 + node_tests + 4 * candidates of the item in the previous evaluation while
 *       the list is the same (n_items, ins_ids given or not, the same kind of entry point, and for the host-pointer entry points
 *       the same ids) and that evaluation succeeded; setting multi_min starts from the leaf products again;
 *       boundary k (k = 1 .. k_use - 1) lies in front of the first item whose half would cross k / k_use of the total cost
 *       (acc + 0.5 * cost[i] < target moves on), so within half an item of its target; then it is clamped so that every one of
 *       the k_use devices has an item at least;
 *       the ranges of the previous evaluation are kept, not cut again, while the list is the same, k_use is and the most loaded
 *       device stays within 15 % of the mean under the new costs (worst * k_use <= 1.15 * total): the chunks of one Jacobian
 *       must see the same ranges to reuse the value pass.  pfc_last_shard_bounds() shows the ranges.
 *     Validated: any number of shard contexts on ONE device (tests/test_gpu_multi_shards.py: 3 and 8, every entry point named
 *     here, idle devices, one dominating item, errors in a middle range).  NOT validated: distinct devices, the peer copies
 *     (hipMemcpyPeerAsync) between them, and the scaling over devices -- no machine with several GPUs has run this code;
 *   - pfc_get_stats sums over the devices; pfc_debug_* go to the device that evaluated the item; pfc_last_parts / _team and
 *     pfc_get_stage_ms report the first device's.
 * Results are those of the single-device handle (counters bit-equal, sums up to their order).
 */
int pfc_create_multi(const int *devices, int n_devices, pfc_handle *out);
int pfc_last_shards(pfc_handle h);   /* devices that took part in the last evaluation (1 for a single-device handle) */
/* Debug view of the last partition: writes bound[0 .. n_used], n_used = pfc_last_shards(h) -- device k evaluated the items
 * [bound[k], bound[k + 1]) of the last evaluation, bound[0] = 0, bound[n_used] = its n_items -- and returns n_used.  A
 * single-device handle writes {0, n_items} and returns 1.  -(PFC_ERR_BAD_ARG) when cap < n_used + 1 or bound is NULL. */
int pfc_last_shard_bounds(pfc_handle h, int *bound, int cap);
void pfc_destroy(pfc_handle h);
const char *pfc_last_error(pfc_handle h);

/*
 * add_contact! -> MeshCache(name, eMesh, tree, body, c_prop) -> addMesh! (src/mechanism_scenario.jl:298-314,258;
 * src/structs.jl:33-45).  Uploads one eMesh (src/geometry/mesh.jl:10-46) and its flattened bin_BB_Tree{OBB}
 * (src/obb/tree_types.jl:1-16, src/obb/box_types.jl:4-9).  Exactly one of tri / tet is non-NULL.
 *   xyz      n_pt x 3        vertex coordinates in the mesh frame
 *   tri      n_tri x 3       (or NULL)      tet  n_tet x 4 (or NULL)      eps  n_pt (tet meshes only)
 *   Ebar     ContactProperties.Ē (tet meshes; ignored for tri meshes)
 *   nodes    n_node entries, node 0 = root: c (x3), e (x3), R (x9 column-major), child (x2), leaf (element index,
 *            or PFC_INTERNAL_NODE)
 * The tree is used as given, like the reference's tree_tree_intersect / BB_BB_intersect (src/obb/tree_types.jl:88-111,
 * src/obb/bb_intersection.jl:2-74): any R is honoured on every node, leaf or internal, by every broadphase kernel; any
 * binary topology over the elements is taken (every internal node has two children in [1, n_node), each node is reached
 * once from the root, leaf ids are element indices: anything else is PFC_ERR_BAD_ARG); a box need not contain its children --
 * a child pair is tested iff its parent pair intersects.  An internal box whose R is not bitwise the identity is always
 * settled by the Float64 test, never by the single-precision filter (whose 24 u radius is derived for axis-aligned internal
 * boxes), so such trees cost broadphase time, not accuracy.
 * Depth limit: for every instruction, depth(tree_1) + depth(tree_2) <= 296 (root = depth 0; the depth-first kernels keep
 * 3 (depth sum + 1) + 3 of their 1 024 stack slots in reserve and need 128 free ones); pfc_finalize returns PFC_ERR_BAD_ARG
 * for a deeper pair ("OBB trees too deep").
 * Returns the mesh id (>= 0) or -(pfc_status).
 */
int pfc_add_mesh(pfc_handle h, int n_pt, const double *xyz, int n_tri, const int *tri, int n_tet, const int *tet,
                 const double *eps, double Ebar, int n_node, const double *node_c, const double *node_e,
                 const double *node_R, const int *node_child, const int *node_leaf);

/*
 * add_friction_regularize! / add_friction_bristle! -> ContactInstructions (src/mechanism_scenario.jl:365-416,
 * :36-49).  id_1 is the triangle mesh (or a tet mesh), id_2 is always a tet mesh (:402-416).
 *   params (PFC_REGULARIZED): [mu_s, mu_d, v_tol]                       (Regularized, :22-34)
 *   params (PFC_BRISTLE):     [mu_s, mu_d, tau, k_bar, magic]           (Bristle, :5-20)
 * n_quad in {1, 2} (:45).  Returns the instruction id (>= 0) or -(pfc_status).
 */
int pfc_add_instruction(pfc_handle h, int id_1, int id_2, double chi, int n_quad, int model, const double *params);

/* finalize! (src/mechanism_scenario.jl:206-231): meshes and instructions become immutable, device tables are
 * built (per-tet zeta transforms of calc_ζ_transforms, src/contact_algorithms_non_friction.jl:158-162, are
 * precomputed here because meshes never change afterwards). */
int pfc_finalize(pfc_handle h);

/*
 * forceAllElasticIntersections! minus the RigidBodyDynamics parts (src/contact_algorithms_non_friction.jl:60-84):
 * evaluates n_items (instruction, pose) items.  ins_ids == NULL means item i uses instruction i.
 *   pose   n_items x 24  x_r2_r1 (R 9 col-major, t 3) then x_r1_r2 (R 9, t 3)   (refreshBodyBodyTransform!, :103-115)
 *   twist  n_items x 6   twist_r2_r1_r2 = [angular; linear]                     (refreshBodyBodyCache!, :125-128)
 *   s      n_items x 6   bristle deflection state (ignored for regularized items; may be NULL if none is bristle)
 *   wrench n_items x 6   OUT wrench on body 2 in frame r2 about its origin, [angular; linear]; zeros if no contact
 *   sdot   n_items x 6   OUT bristle state derivative (friction.jl:134; no contact: -s/tau, :77-81); zeros if regularized
 *   counts n_items x 4   OUT {OBB node tests, candidate pairs, pairs with a non-empty polygon, traction points}
 *                        (may be NULL)
 * Synchronous.  Work-list overflows are handled internally (grow + re-run), mirroring VectorCache doubling
 * (src/obb/vector_cache.jl:13-17).
 */
int pfc_eval(pfc_handle h, int n_items, const int *ins_ids, const double *pose, const double *twist,
             const double *s, double *wrench, double *sdot, int *counts);

/*
 * Same evaluation with every buffer resident in device memory (HBM) and no host synchronisation: kernels are
 * enqueued on `stream` (a hipStream_t; NULL = the handle's own stream).  d_ins_ids may be NULL.  Call
 * pfc_check() afterwards: it synchronises and returns PFC_ERR_OVERFLOW (after growing the work lists) if the
 * evaluation must be re-issued.
 */
int pfc_eval_device(pfc_handle h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist,
                    const double *d_s, double *d_wrench, double *d_sdot, int *d_counts, void *stream);
int pfc_check(pfc_handle h);

/*
 * The same evaluation on ForwardDiff.Dual numbers: what forceAllElasticIntersections! does when calcXd! runs on
 * MechanismScenario.dual (Dual{Nothing,Float64,N_chunk}, src/mechanism_scenario.jl:187) for Radau's Jacobian
 * (src/radau/radau_functions.jl:2-40).  Values as pfc_eval; in addition, for each of n_dir (1..16) seed directions,
 * the partials of every input and of every output:
 *   d_pose   n_items x n_dir x 24   partials of pose (same packing as pose)
 *   d_twist  n_items x n_dir x 6    d_s  n_items x n_dir x 6 (or NULL = zeros)
 *   d_wrench n_items x n_dir x 6    OUT partials of wrench     d_sdot  n_items x n_dir x 6   OUT partials of sdot
 * The candidate pairs come from the value pass (the intersection does not depend on partials,
 * src/contact_algorithms_non_friction.jl:95); every branch compares values, as ForwardDiff's comparisons do.  The one
 * step that is not the reference's operation sequence is eigen!(Hermitian{Dual}) (src/contact_algorithms_friction.jl:88,
 * GenericLinearAlgebra): the partials of K̄^{-1/2} are its analytic Frechet derivative ("Dual path").
 * An (item, direction) whose 36 seed components (d_pose 24, d_twist 6, d_s 6) are all zero has zero partials by
 * linearity and is not evaluated: the cost of a chunk follows the instructions its seeded state variables touch.
 * Host buffers, synchronous.
 */
int pfc_eval_dual(pfc_handle h, int n_items, int n_dir, const int *ins_ids, const double *pose, const double *twist,
                  const double *s, const double *d_pose, const double *d_twist, const double *d_s, double *wrench,
                  double *sdot, double *d_wrench, double *d_sdot, int *counts);

/*
 * pfc_eval_dual with the broadphase run on a pose of its own.  The reference culls with the transforms of m.float's state
 * whatever scenario is being evaluated (calcTriTetIntersections!: `refreshBodyBodyTransform!(m, m.float, c_ins)`,
 * src/contact_algorithms_non_friction.jl:94-101), and m.float holds what the last Float64 calcXd! left there
 * (src/extensions.jl:21) -- in Radau's Jacobian that is NOT value.(x_dual) in general.  bp_pose (n_items x 24, the packing of
 * pose; only the x_r1_r2 half is read) is that pose: typically the `pose` array of the host's last pfc_eval.  NULL: the
 * candidates come from pose itself, i.e. pfc_eval_dual.  The narrowphase, and every output, is evaluated at pose.
 */
int pfc_eval_dual_bp(pfc_handle h, int n_items, int n_dir, const int *ins_ids, const double *pose, const double *bp_pose,
                     const double *twist, const double *s, const double *d_pose, const double *d_twist, const double *d_s,
                     double *wrench, double *sdot, double *d_wrench, double *d_sdot, int *counts);

/*
 * pfc_eval_dual with every buffer resident in device memory and no host synchronisation (the Dual sibling of
 * pfc_eval_device; Radau's Jacobian evaluations are half of its calls, src/radau/radau_functions.jl:2-14): value pass and
 * Dual passes are enqueued back to back on `stream`.  The Dual polygons kept between the passes are sized from the
 * previous Dual evaluation of the handle; pfc_check() synchronises and returns PFC_ERR_OVERFLOW if a work list or that
 * speculation fell short (buffers have grown: re-issue).  d_ds may be NULL (zeros); d_ins_ids and d_counts may be NULL.
 */
int pfc_eval_dual_device(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const double *d_pose,
                         const double *d_twist, const double *d_s, const double *d_dpose, const double *d_dtwist,
                         const double *d_ds, double *d_wrench, double *d_sdot, double *d_dwrench, double *d_dsdot,
                         int *d_counts, void *stream);
/* ... with the broadphase pose of pfc_eval_dual_bp in device memory (d_bp_pose n_items x 24, may be NULL). */
int pfc_eval_dual_device_bp(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const double *d_pose,
                            const double *d_bp_pose, const double *d_twist, const double *d_s, const double *d_dpose,
                            const double *d_dtwist, const double *d_ds, double *d_wrench, double *d_sdot, double *d_dwrench,
                            double *d_dsdot, int *d_counts, void *stream);

/*
 * Further seed directions AT THE POINT OF THE PREVIOUS pfc_eval_dual_device evaluation of this handle: the chunks of one
 * Jacobian (update of the Radau iteration matrix: ceil(NX / N_chunk) Dual evaluations with the same values and different
 * partials, src/radau/radau_functions.jl:2-14).  Only the Dual passes run; candidates, contributing pairs and per-item
 * results of that evaluation's value pass are reused, its value outputs are not written again.  n_dir may differ from the
 * first call.  Requires that pfc_check() returned PFC_OK for that evaluation and that nothing else was evaluated on the
 * handle since (PFC_ERR_STATE otherwise); follow with pfc_check() (synchronises; no speculation: it cannot ask for a
 * re-issue).  An evaluation of zero items through a device-pointer entry point is an evaluation too: it drops an unchecked
 * call and ends this reuse, on single- and multi-device handles alike.  pfc_eval_dual applies the same reuse by itself when the value inputs of a call equal, bit for bit, those
 * of the previous call (option "dual_reuse", default 1).
 */
int pfc_eval_dual_device_more(pfc_handle h, int n_dir, const double *d_dpose, const double *d_dtwist, const double *d_ds,
                              double *d_dwrench, double *d_dsdot, void *stream);

/*
 * The contact Jacobian of every item AT THE POINT OF THE LAST CHECKED pfc_eval_dual_device[_bp] EVALUATION of this handle.  Every
 * branch of the Dual passes compares values (the clip, max(0, 1 + chi edot), the friction ramps, the eigenvalue clamp) and the
 * Frechet derivative of K̄^{-1/2} is linear in dK, so at one value point an item's partials are one matrix times its seeds:
 *   [d_wrench; d_sdot] (12 x n_dir) = L (12 x 36) . [d_pose 24; d_twist 6; d_s 6] (36 x n_dir).
 *   d_L  n_items x 12 x 36   OUT row-major per item: row r = output r (wrench [ang; lin] 0..5, then sdot 6..11), column k = input k
 *                            (the 24 pose numbers in pfc_eval's packing 0..23, twist 24..29, s 30..35).  The pose columns are the
 *                            contact stiffness, the twist columns the damping.
 * Three Dual passes (16 + 16 + 4 unit-seed directions) run on the kept value pass, as pfc_eval_dual_device_more runs its one: the
 * columns are bit for bit the partials _more returns for those unit seeds.  Precondition, state and check as _more: PFC_ERR_STATE
 * without a checked Dual evaluation to extend; follow with pfc_check(); the handle is left as _more leaves it (further _more calls and
 * pfc_local_jacobian_device at the same point still work).  Multi-device handles: each device builds the rows of its items, d_L lives
 * on the first device.
 * Flat patches: on a default handle each Dual pass forms K from its own atomically summed Dual sums; where decompose_K! clamps an
 * eigenvalue (src/contact_algorithms_friction.jl:92) two passes can take different clamp decisions and their partials then differ
 * by O(1) -- L's columns come from three passes, a chunk of _more from one.  Under option fixed_order every pass takes the value
 * pass's K and a fixed summation order: L equals _more's partials for the same unit seeds byte for byte.
 */
int pfc_local_jacobian_device(pfc_handle h, double *d_L, void *stream);
/* The host-buffer, synchronous one-shot: the value pass of pfc_eval at (ins_ids, pose, twist, s) -- a Dual evaluation whose seeds are
 * all zero -- then L (n_items x 12 x 36).  Arguments as pfc_eval, plus L; counts may be NULL.  Work-list overflows are handled
 * internally.  The call counts as a Dual evaluation: pfc_eval_dual_device_more and pfc_local_jacobian_device may follow at its point. */
int pfc_local_jacobian(pfc_handle h, int n_items, const int *ins_ids, const double *pose, const double *twist, const double *s,
                       double *wrench, double *sdot, double *L, int *counts);

/*
 * Further seed chunks from L: d_wrench / d_sdot of every (item, direction) = L_item . [d_pose; d_twist; d_s], with exactly the
 * layouts of pfc_eval_dual_device_more (n_dir 1..16; d_ds may be NULL = zeros), so the result goes straight into
 * pfc_scatter_generalized_dual_device.  A key whose 36 seeds are all zero gets exact zeros without reading L (an item without a
 * nonzero key reads no L at all); NaN seeds propagate.  L is caller data: the call reads and changes no evaluation state of the handle,
 * so it stays valid after later evaluations and pfc_set_option -- the same flat-patch caveat as pfc_local_jacobian_device applies to
 * the L it is given.  d_L must be 16-byte aligned.  Enqueued on `stream` (NULL = the handle's own) without a synchronisation and
 * needs no pfc_check.  Multi-device handles: the first device, over all items.  Each output is one FMA chain over the 36 columns in
 * order: the same bytes on every call.
 */
int pfc_apply_local_jacobian_device(pfc_handle h, int n_items, int n_dir, const double *d_L, const double *d_dpose,
                                    const double *d_dtwist, const double *d_ds, double *d_dwrench, double *d_dsdot, void *stream);
/* The same with host buffers, synchronous. */
int pfc_apply_local_jacobian(pfc_handle h, int n_items, int n_dir, const double *L, const double *d_pose, const double *d_twist,
                             const double *d_s, double *d_wrench, double *d_sdot);

/*
 * eMesh_to_tree (src/geometry/blob_types.jl:136-173) on the host: builds the flattened binary OBB tree that
 * pfc_add_mesh takes.  method PFC_TREE_BLOB follows the reference (bottom-up merging of face/edge-adjacent blobs by
 * marginal cost :74-134, median-split top-down over the remaining blobs src/geometry/top_down.jl:10-32, tight leaf
 * boxes src/obb/obb_construction.jl:13-41); PFC_TREE_MEDIAN skips the bottom-up phase (pure top_down.jl).  Equal-cost
 * merges are ordered by (cost, blob key); Julia's PriorityQueue order among ties is not specified, so trees are
 * quality-equivalent rather than node-identical to Julia-built ones.
 *   elem   n_elem x arity (3: triangles, 4: tets), 0-based; eps per point (tets only, may be NULL for triangles)
 *   node_* OUT arrays sized for 2*n_elem-1 nodes: c (x3), e (x3), R (x9 column-major), child (x2), leaf (x1)
 * Returns the node count (2*n_elem-1) or a negative pfc_status; message via pfc_tree_last_error().  Reference
 * errors kept: "three triangles share the same edge", "three tetrahedrons share the same face", open triangle
 * surfaces ("not implemented error: disconnected mesh", :156), "inverted tet".
 */
enum { PFC_TREE_BLOB = 0, PFC_TREE_MEDIAN = 1 };
int pfc_build_tree(int n_pt, const double *pt, int n_elem, int arity, const int *elem, const double *eps, int method,
                   double *node_c, double *node_e, double *node_R, int *node_child, int *node_leaf);
const char *pfc_tree_last_error(void);

/*
 * addGeneralizedForcesThirdLaw! for every item (src/contact_algorithms_non_friction.jl:267-286): the item's wrench is
 * moved to the world frame with x_rw_r2 (RigidBodyDynamics transform(wrench, .)) and projected on the geometric
 * Jacobians of the two bodies (torque!), f[scene] += J_2' w - J_1' w.
 *   wrench  n_items x 6   [angular; linear], as returned by pfc_eval
 *   x_w_r2  n_items x 12  x_rw_r2: R (9, column-major) then t (3)
 *   body_1, body_2        body index of mesh_1 / mesh_2 per item, or -1 for a body without Jacobian (root: the
 *                         addGeneralizedForcesExternal!(..., jac::Nothing, ...) method, :275-279)
 *   scene   n_items       scene (mechanism) index per item, or NULL for a single mechanism
 *   jac     n_body x nv x 6   per body the 6 x nv geometric Jacobian, column-major (rows 0..2 angular, 3..5 linear)
 *   f_out   n_scene x nv  OUT f_generalized contribution of the contacts (overwritten)
 * Host buffers, synchronous.
 */
int pfc_scatter_generalized(pfc_handle h, int n_items, const double *wrench, const double *x_w_r2, const int *body_1,
                            const int *body_2, const int *scene, int n_scene, int n_body, int nv, const double *jac,
                            double *f_out);

/*
 * pfc_scatter_generalized with every buffer resident in device memory, enqueued on `stream` without a host
 * synchronisation: the wrenches are the ones pfc_eval_device left in HBM, f_generalized stays there for the next consumer
 * ("keep f_generalized resident").  accumulate = 0: d_f (n_scene x nv) is cleared first; 1: the
 * contact forces are added to what d_f holds (the reference adds to the f_generalized of the other force sources,
 * src/contact_algorithms_non_friction.jl:40-52).  Body / scene ids are NOT range-checked here (they are device data): an id
 * outside [-1, n_body) / [0, n_scene) is undefined behaviour, as with any device pointer of the wrong size.  d_scene may
 * be NULL (one mechanism).
 */
int pfc_scatter_generalized_device(pfc_handle h, int n_items, const double *d_wrench, const double *d_x_w_r2, const int *d_body_1,
                                   const int *d_body_2, const int *d_scene, int n_scene, int nv, const double *d_jac, double *d_f,
                                   int accumulate, void *stream);

/*
 * addGeneralizedForcesThirdLaw! on Dual numbers (src/contact_algorithms_non_friction.jl:267-286 as the reference runs it in
 * each Jacobian chunk of the Radau iteration matrix, src/radau/radau_functions.jl:2-14): the wrench, x_rw_r2 and the geometric
 * Jacobians (refreshJacobians!, :86-92) carry partials, and f_generalized gets values and partials.  Arguments as
 * pfc_scatter_generalized, plus, for n_dir (1..16) seed directions:
 *   d_wrench  n_items x n_dir x 6          partials of the wrenches, as pfc_eval_dual[_device][_more] writes them
 *   d_x_w_r2  n_items x n_dir x 12         partials of x_rw_r2, or NULL (constant: the same bytes as an array of zeros)
 *   d_jac     n_body x n_dir x nv x 6      partials of the Jacobians, or NULL (constant, likewise)
 *   f_out     n_scene x nv                 OUT values (overwritten), or NULL
 *   d_f_out   n_scene x n_dir x nv         OUT partials (overwritten): one f-vector per direction
 * Order: every output entry (scene, direction, coordinate) is summed over the scene's items in ascending item order,
 * +tau(body_2) then -tau(body_1), as the reference loops over its instructions; every product of a value and a partial follows
 * ForwardDiff (d(a b) = da b + a db).  No atomics: f_out equals pfo_scatter_generalized's result bit for bit (and
 * pfc_scatter_generalized's up to summation order), and both outputs are the same bytes for the same inputs on every call,
 * handle, stream and entry point.  Scene ids need not be contiguous.  Limits: n_scene * n_items < 2^31 (PFC_ERR_BAD_ARG).
 * Host buffers, synchronous; body and scene ids are range-checked.
 */
int pfc_scatter_generalized_dual(pfc_handle h, int n_items, int n_dir, const double *wrench, const double *d_wrench,
                                 const double *x_w_r2, const double *d_x_w_r2, const int *body_1, const int *body_2,
                                 const int *scene, int n_scene, int n_body, int nv, const double *jac, const double *d_jac,
                                 double *f_out, double *d_f_out);

/*
 * pfc_scatter_generalized_dual with every buffer in device memory, enqueued on `stream` without a host synchronisation: the
 * Dual wrenches pfc_eval_dual_device / pfc_eval_dual_device_more left in HBM are projected where they are, chunk after chunk on
 * one stream.  accumulate = 0: d_f and d_df are overwritten; 1: the contact terms are added onto what they hold (that content is
 * the first term of every sum).  d_f may be NULL (partials only); d_scene may be NULL (one mechanism).  Body ids are not
 * range-checked (device data, as in pfc_scatter_generalized_device); an item whose scene id lies outside [0, n_scene) is left
 * out.  Multi-device handles: the first device.  The call keeps work buffers in the handle: calls on different streams must be
 * ordered by the caller.
 */
int pfc_scatter_generalized_dual_device(pfc_handle h, int n_items, int n_dir, const double *d_wrench_val, const double *d_dwrench,
                                        const double *d_x_w_r2, const double *d_dx_w_r2, const int *d_body_1, const int *d_body_2,
                                        const int *d_scene, int n_scene, int nv, const double *d_jac, const double *d_djac,
                                        double *d_f, double *d_df, int accumulate, void *stream);

/*
 * Contact items from body states: refreshBodyBodyTransform! / refreshBodyBodyCache! (src/contact_algorithms_non_friction.jl:103-134)
 * on the device, for rigid bodies whose world poses and twists the host (or another kernel) keeps in HBM -- the front of the chain
 * body states -> items -> pfc_eval_device -> pfc_scatter_generalized_device, which then runs on one stream without a host copy.
 *
 * pfc_set_instruction_bodies binds instruction `ins` to the bodies of its mesh_1 / mesh_2 (MeshCache.BodyID; meshes are given in
 * their body's frame).  -1 is the world: identity pose, zero twist, no Jacobian (pfc_scatter_generalized's convention).  Allowed
 * before and after pfc_finalize (before: any id >= 0; after: an instruction of the scenario); a second call overwrites the first and
 * takes effect with the next call below.  The first of them after a binding uploads the table (one stream synchronisation).
 * Multi-device handles keep the table on their first device.
 */
int pfc_set_instruction_bodies(pfc_handle h, int ins, int body_1, int body_2);

/*
 * One kernel, one item per lane, enqueued on `stream` (NULL = the handle's own) without a host synchronisation:
 *   d_ins_ids    n_items, or NULL: item i uses instruction i           d_scene  n_items, or NULL: scene 0
 *   d_x_w_b      n_scene n_body x 12   world pose of body b of scene s at row s n_body + b: R (9, column-major), t (3)
 *   d_twist_w_b  n_scene n_body x 6    its twist [angular; linear] in world about the world origin (RigidBodyDynamics' twist_wrt_world)
 *   d_pose       n_items x 24  OUT x_r2_r1 then x_r1_r2, pfc_eval's packing       d_twist  n_items x 6  OUT twist_r2_r1_r2
 *   d_x_w_r2     n_items x 12  OUT x_rw_r2, pfc_scatter_generalized's packing (the pose of body 2, copied)
 *   d_body_1, d_body_2  n_items  OUT the bound bodies; with d_scene given offset by scene n_body, so that they index a Jacobian array
 *                       of n_scene n_body bodies; -1 stays -1
 * Any OUT pointer may be NULL (not wanted, not written).  The arithmetic is plain Float64, every 3-term dot product summed left to
 * right without fma, the world going through the same expressions with R = I, t = 0:
 *   R2w = R_w2', t2w = -(R2w t_w2);  R21 = R2w R_w1, t21 = (R2w t_w1) + t2w;  R12 = R21', t12 = -(R12 t21);
 *   tw = tw_2 - tw_1;  ang = R2w tw_ang;  lin = (R2w tw_lin) + t2w x ang
 * -- the same bytes on every call, handle and entry point.  The call is NOT an evaluation: a kept value pass, Dual reuse,
 * pfc_check and pfc_last_* are as they were.  n_items = 0 is a no-op.
 * PFC_ERR_STATE: before pfc_finalize; an instruction without bodies (the message names it) -- the ids are device data and are not
 * read by the host, so without d_ins_ids the instructions 0 .. n_items - 1 must be bound, with d_ins_ids every instruction of the
 * scenario.  PFC_ERR_BAD_ARG: such an instruction bound to a body >= n_body.  Instruction and scene ids are not range-checked (the
 * rule of pfc_scatter_generalized_device), but no item follows one out of range: such an item writes nothing.
 */
int pfc_items_from_bodies_device(pfc_handle h, int n_items, const int *d_ins_ids, const int *d_scene, int n_scene, int n_body,
                                 const double *d_x_w_b, const double *d_twist_w_b, double *d_pose, double *d_twist, double *d_x_w_r2,
                                 int *d_body_1, int *d_body_2, void *stream);
/* The same with host buffers, synchronous.  Only the instructions the items use must be bound; instruction, scene and body ids are
 * range-checked (PFC_ERR_BAD_ARG, nothing is written). */
int pfc_items_from_bodies(pfc_handle h, int n_items, const int *ins_ids, const int *scene, int n_scene, int n_body, const double *x_w_b,
                          const double *twist_w_b, double *pose, double *twist, double *x_w_r2, int *body_1, int *body_2);

/*
 * pfc_items_from_bodies_device followed by exactly pfc_eval_device on the same stream, reading the d_pose / d_twist the kernel
 * wrote (both required here; the other three item outputs may be NULL).  The item buffers are the caller's: the scatter needs three
 * of them, and the handle allocates nothing per evaluation.  pfc_check() afterwards as after pfc_eval_device; on PFC_ERR_OVERFLOW
 * re-issue this call (the items are formed again, to the same bytes).
 */
int pfc_eval_bodies_device(pfc_handle h, int n_items, const int *d_ins_ids, const int *d_scene, int n_scene, int n_body,
                           const double *d_x_w_b, const double *d_twist_w_b, const double *d_s, double *d_pose, double *d_twist,
                           double *d_x_w_r2, int *d_body_1, int *d_body_2, double *d_wrench, double *d_sdot, int *d_counts, void *stream);
/* The host-buffer form: pfc_items_from_bodies, then pfc_eval.  pose, twist, x_w_r2, body_1, body_2 are optional OUT arguments
 * (NULL: the items are not returned).  Synchronous. */
int pfc_eval_bodies(pfc_handle h, int n_items, const int *ins_ids, const int *scene, int n_scene, int n_body, const double *x_w_b,
                    const double *twist_w_b, const double *s, double *pose, double *twist, double *x_w_r2, int *body_1, int *body_2,
                    double *wrench, double *sdot, int *counts);

/*
 * Dual seeds of the items from body states: refreshBodyBodyTransform! / refreshBodyBodyCache! as the reference runs them on the Dual
 * state of a Jacobian chunk (src/radau/radau_functions.jl:2-14), where the bodies' world poses and twists carry partials -- the front
 * of the chain body states + partials -> seeds -> pfc_eval_dual_device[_more] -> pfc_scatter_generalized_dual_device.  One kernel, one
 * lane per (item, direction), enqueued on `stream` (NULL = the handle's own) without a host synchronisation.  Arguments as
 * pfc_items_from_bodies_device, plus, for n_dir (1..16, else PFC_ERR_BAD_ARG) seed directions:
 *   d_dx_w_b      n_scene n_body x n_dir x 12   partials of d_x_w_b, direction dir of body b of scene s at row (s n_body + b) n_dir + dir
 *   d_dtwist_w_b  n_scene n_body x n_dir x 6    partials of d_twist_w_b, likewise
 *                 each may be NULL: zeros, the same bytes as an array of zeros (the chunk that seeds only velocities or only
 *                 configurations)
 *   d_dpose       n_items x n_dir x 24  OUT partials of x_r2_r1 then x_r1_r2, pfc_eval_dual_device's d_dpose
 *   d_dtwist      n_items x n_dir x 6   OUT partials of twist_r2_r1_r2, its d_dtwist
 *   d_dx_w_r2     n_items x n_dir x 12  OUT partials of x_rw_r2, pfc_scatter_generalized_dual_device's d_dx_w_r2 (the partials of body
 *                 2's pose, gathered; zeros for the world)
 * Any OUT pointer may be NULL (not wanted, not written).  The arithmetic is the statement of pfc_items_from_bodies_device on
 * (value, partial) numbers with ForwardDiff's rules -- sums and differences componentwise, d(a b) = da b + a db, no fma -- and the
 * world going through it with R = I, t = 0, a zero twist and zero partials: the same bytes on every call, handle and entry point.
 * The call is NOT an evaluation: a kept value pass, Dual reuse, pfc_check and pfc_last_* are as they were (a pfc_eval_dual_device_more
 * may still follow the evaluation before it).  n_items = 0 is a no-op.  States, errors and the treatment of ids are those of
 * pfc_items_from_bodies_device: an item with an instruction or scene id out of range writes nothing.  Multi-device handles: the first
 * device.
 */
int pfc_dual_seeds_from_bodies_device(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene,
                                      int n_scene, int n_body, const double *d_x_w_b, const double *d_twist_w_b,
                                      const double *d_dx_w_b, const double *d_dtwist_w_b,
                                      double *d_dpose, double *d_dtwist, double *d_dx_w_r2, void *stream);
/* The same with host buffers, synchronous.  Only the instructions the items use must be bound; instruction, scene and body ids are
 * range-checked (PFC_ERR_BAD_ARG, nothing is written). */
int pfc_dual_seeds_from_bodies(pfc_handle h, int n_items, int n_dir, const int *ins_ids, const int *scene,
                               int n_scene, int n_body, const double *x_w_b, const double *twist_w_b,
                               const double *d_x_w_b, const double *d_twist_w_b, double *d_pose, double *d_twist, double *d_x_w_r2);

/*
 * pfc_items_from_bodies_device, pfc_dual_seeds_from_bodies_device, then exactly pfc_eval_dual_device on the same stream, reading the
 * d_pose / d_twist / d_dpose / d_dtwist the kernels wrote (all four required here; d_x_w_r2, d_body_1, d_body_2 and d_dx_w_r2 may be
 * NULL).  d_s / d_ds as pfc_eval_dual_device.  The item and seed buffers are the caller's: the Dual scatter needs four of them, and
 * the handle allocates nothing per evaluation.  pfc_check() afterwards as after pfc_eval_dual_device; on PFC_ERR_OVERFLOW re-issue
 * this call (items and seeds are formed again, to the same bytes).
 */
int pfc_eval_dual_bodies_device(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene,
                                int n_scene, int n_body, const double *d_x_w_b, const double *d_twist_w_b,
                                const double *d_dx_w_b, const double *d_dtwist_w_b, const double *d_s, const double *d_ds,
                                double *d_pose, double *d_twist, double *d_x_w_r2, int *d_body_1, int *d_body_2,
                                double *d_dpose, double *d_dtwist, double *d_dx_w_r2,
                                double *d_wrench, double *d_sdot, double *d_dwrench, double *d_dsdot, int *d_counts, void *stream);
/*
 * The later chunks of a Jacobian at the kept point, from body-state partials: pfc_dual_seeds_from_bodies_device, then exactly
 * pfc_eval_dual_device_more on the d_dpose / d_dtwist it wrote (both required; d_dx_w_r2 may be NULL).  The value states are read
 * again (the partials of a product need them) but no value output is written.  Single-device handles check _more's preconditions before
 * anything is launched -- PFC_ERR_STATE without a checked pfc_eval_dual_device evaluation to extend, PFC_ERR_BAD_ARG if n_items is not
 * that evaluation's -- and then write nothing.  Multi-device handles form the seeds on the first device and then return _more's own
 * status: there the seed buffers are written even where _more refuses.  Follow with pfc_check() as after pfc_eval_dual_device_more.
 */
int pfc_eval_dual_bodies_device_more(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene,
                                     int n_scene, int n_body, const double *d_x_w_b, const double *d_twist_w_b,
                                     const double *d_dx_w_b, const double *d_dtwist_w_b, const double *d_ds,
                                     double *d_dpose, double *d_dtwist, double *d_dx_w_r2, double *d_dwrench, double *d_dsdot, void *stream);

/*
 * Kinematics from joint states: what transform_to_root / twist_wrt_world (src/contact_algorithms_non_friction.jl:109-110,125-126) and
 * refreshJacobians! (:86-92) give the reference per evaluation -- the bodies' world poses, twists and geometric Jacobians -- formed on
 * the device from the state vector (q, v), the front of the chain state -> body states -> items -> pfc_eval_device ->
 * pfc_scatter_generalized_device.  The value path; its Dual sibling is pfc_kinematics_dual_device below.
 *
 * pfc_set_mechanism gives the tree.  Body b is the successor of joint b; parent[b] lies in [-1, b), -1 is the world, so the order is
 * topological.  x_p_j (n_body x 12) is the joint's joint_pose -- the frame before the joint in the parent body's frame, R (9,
 * column-major) then t, pfc_scatter_generalized's packing -- and the body's frame is the joint's frame after.  axis (n_body x 3) is
 * given in the joint frame and read for revolute and prismatic joints only.  Joint types:
 */
#define PFC_JOINT_FIXED 0          /* no coordinates */
#define PFC_JOINT_REVOLUTE 1       /* 1 q (angle), 1 v */
#define PFC_JOINT_PRISMATIC 2      /* 1 q (displacement), 1 v */
#define PFC_JOINT_FLOATING_MRP 3   /* 6 q = [modified Rodrigues parameters (3); translation (3)], 6 v = [omega; v] in the frame after:
                                      RigidBodyDynamics' SPQuatFloating */
/*
 * Coordinate offsets are cumulative in body order (RigidBodyDynamics' tree order when the host numbers bodies in attach order).
 * Allowed before and after pfc_finalize; a second call replaces the first and takes effect with the next call below, the first of
 * which uploads the tables (one stream synchronisation).  Multi-device handles keep the tables on their first device.
 * PFC_ERR_BAD_ARG, the message naming the body: n_body < 1, a parent outside [-1, b), an unknown joint type, a null table, a revolute
 * or prismatic axis with | |a|^2 - 1 | > 1e-12.  pfc_mechanism_sizes returns n_body, nq, nv (any pointer may be NULL; PFC_ERR_STATE
 * before pfc_set_mechanism).
 */
int pfc_set_mechanism(pfc_handle h, int n_body, const int *parent, const int *joint_type, const double *x_p_j, const double *axis);
int pfc_mechanism_sizes(pfc_handle h, int *n_body, int *nq, int *nv);

/*
 * Two kernels enqueued on `stream` (NULL = the handle's own) without a host synchronisation:
 *   d_q          n_scene x nq             d_v  n_scene x nv (may be NULL when d_twist_w_b is: zeros)
 *   d_x_w_b      n_scene n_body x 12  OUT world pose of body b of scene s at row s n_body + b, pfc_items_from_bodies_device's d_x_w_b
 *   d_twist_w_b  n_scene n_body x 6   OUT its twist [angular; linear] in world about the world origin, likewise
 *   d_jac        n_scene n_body x nv x 6  OUT the geometric Jacobians, pfc_scatter_generalized_device's d_jac for the scene-offset
 *                body ids pfc_items_from_bodies_device writes
 * Any OUT pointer may be NULL: it is not written, and the work it alone needs is not launched.  The arithmetic is plain Float64, every
 * 3-term dot product summed left to right without fma, a translation added last; the world goes through the same expressions with
 * R = I, t = 0 and a zero twist:
 *   joint transform X_j(q).  fixed: (I, 0).  prismatic: R = I, t_r = a_r d.
 *     floating: a2 = (p0 p0 + p1 p1) + p2 p2; den = a2 + 1; w = (1 - a2) / den; x = (2 p0) / den, y, z likewise;
 *       R00 = ((ww + xx) - yy) - zz   R01 = 2 (xy - zw)             R02 = 2 (xz + yw)
 *       R10 = 2 (xy + zw)             R11 = ((ww - xx) + yy) - zz   R12 = 2 (yz - xw)
 *       R20 = 2 (xz - yw)             R21 = 2 (yz + xw)             R22 = ((ww - xx) - yy) + zz;     t = q[3..6)
 *     revolute: c = cos q, s = sin q, c1 = 1 - c; R_rr = (c1 a_r) a_r + c;
 *       R10 = (c1 a0) a1 + s a2, R01 = (c1 a0) a1 - s a2;  R20 = (c1 a0) a2 - s a1, R02 = (c1 a0) a2 + s a1;
 *       R21 = (c1 a1) a2 + s a0, R12 = (c1 a1) a2 - s a0;  t = 0
 *   pose.  A = x_p_j o X_j: R_A = R_pj R_j, t_A = (R_pj t_j) + t_pj;  x_w_b = x_w_parent o A: R = R_wp R_A, t = (R_wp t_A) + t_wp
 *   twist.  joint twist in the frame after: floating [omega; v], revolute [a qdot; 0], prismatic [0; a qdot], fixed 0;
 *     ang_w = R_wb ang_j;  lin_w = (R_wb lin_j) + t_wb x ang_w;  tw_b = tw_parent + [ang_w; lin_w] elementwise
 *   motion-subspace column of velocity coordinate c, owned by joint b, in world.  floating k < 3: ang = R_wb[:,k], lin = t_wb x ang;
 *     k >= 3: ang = 0, lin = R_wb[:,k-3];  revolute: ang = R_wb a, lin = t_wb x ang;  prismatic: ang = 0, lin = R_wb a
 *   Jacobian of body b (the root -> b path of refreshJacobians!): column c is that column if the owning joint lies on the path, +0.0
 *     six times otherwise.  A body behind fixed joints only gets an all-zero Jacobian (the scatter adds zeros: the reference's
 *     jac::Nothing for the root).
 * -- the same bytes on every call, handle and entry point.  The call is NOT an evaluation: a kept value pass, Dual reuse, pfc_check
 * and pfc_last_* are as they were.  n_scene = 0 is a no-op.  PFC_ERR_STATE before pfc_set_mechanism.  The call keeps the columns in a
 * handle buffer that grows on demand only: calls on different streams must be ordered by the caller.  Multi-device handles: the first
 * device.
 */
int pfc_kinematics_device(pfc_handle h, int n_scene, const double *d_q, const double *d_v, double *d_x_w_b, double *d_twist_w_b,
                          double *d_jac, void *stream);
/* The same with host buffers, synchronous: the same kernels, the same bytes. */
int pfc_kinematics(pfc_handle h, int n_scene, const double *q, const double *v, double *x_w_b, double *twist_w_b, double *jac);

/*
 * pfc_kinematics_device, then exactly pfc_eval_bodies_device, then pfc_scatter_generalized_device with accumulate = 0, on one stream,
 * with n_body and nv of the mechanism: the only per-step upload left is the state vector.  d_f (n_scene x nv) = NULL skips the scatter.
 * All buffers are the caller's and all are required but d_ins_ids, d_scene, d_s, d_counts (as pfc_eval_bodies_device) and d_f; with d_f
 * also d_jac, d_x_w_r2, d_body_1 and d_body_2.  pfc_check() afterwards as after pfc_eval_device; on PFC_ERR_OVERFLOW d_f is undefined
 * and the call is re-issued (the items are formed again, to the same bytes).  States and errors are those of the parts, checked
 * before anything is launched; PFC_ERR_BAD_ARG if an instruction the items use is bound to a body >= n_body of the mechanism.  There
 * is no accumulate variant: a host that accumulates calls the parts.
 */
int pfc_eval_state_device(pfc_handle h, int n_items, const int *d_ins_ids, const int *d_scene, int n_scene,
                          const double *d_q, const double *d_v, const double *d_s,
                          double *d_x_w_b, double *d_twist_w_b, double *d_jac,
                          double *d_pose, double *d_twist, double *d_x_w_r2, int *d_body_1, int *d_body_2,
                          double *d_wrench, double *d_sdot, int *d_counts, double *d_f, void *stream);
/* The host-buffer form: pfc_kinematics, pfc_eval_bodies, pfc_scatter_generalized.  x_w_b, twist_w_b, jac, pose, twist, x_w_r2, body_1,
 * body_2 are optional OUT arguments (NULL: not returned), and so is f (NULL: no scatter).  Synchronous. */
int pfc_eval_state(pfc_handle h, int n_items, const int *ins_ids, const int *scene, int n_scene,
                   const double *q, const double *v, const double *s,
                   double *x_w_b, double *twist_w_b, double *jac,
                   double *pose, double *twist, double *x_w_r2, int *body_1, int *body_2,
                   double *wrench, double *sdot, int *counts, double *f);

/*
 * Forward dynamics from joint states: what configuration_derivative!, mass_matrix!, dynamics_bias!, sum_all_forces!, cholesky! and
 * ldiv! (src/contact_algorithms_non_friction.jl:18-52) give the reference per evaluation -- qdot, the mass matrix H, the bias c and
 * vdot = H^-1 ((f - c) + tau) -- formed on the device, so that xx = [qdot; vdot; sdot] follows from x = [q; v; s] without a host that
 * owns a dynamics library.  The value path; the Dual siblings are pfc_dynamics_dual_device and pfc_accelerations_dual_device below.
 *
 * pfc_set_inertia gives the bodies' inertias and gravity.  inertia (n_body x 13) holds per body RigidBodyDynamics' SpatialInertia in
 * the body's own frame: moment (9, column-major, about the frame origin), cross_part = m com (3), mass (1).  gravity (3) is the
 * gravitational acceleration in world, e.g. (0, 0, -9.81).  Allowed only after pfc_set_mechanism (PFC_ERR_STATE before it); a later
 * pfc_set_mechanism drops the inertias.  PFC_ERR_BAD_ARG, the message naming the body: n_body different from the mechanism's, a null
 * table, a negative or non-finite mass, a non-finite entry, a moment with |M_rc - M_cr| > 1e-12 max|M|.  Zero mass is allowed (a dummy
 * body behind a fixed joint).  A failed call leaves the previous inertias in place.  The table is uploaded with the mechanism's, by
 * the first call that needs it (one stream synchronisation), on the first device of a multi-device handle.
 */
int pfc_set_inertia(pfc_handle h, int n_body, const double *inertia, const double *gravity);

/*
 * One kernel (one 64-lane workgroup per scene) enqueued on `stream` (NULL = the handle's own) without a host synchronisation:
 *   d_q, d_v     as pfc_kinematics_device           d_x_w_b, d_twist_w_b  pfc_kinematics_device's outputs for the same (q, v)
 *   d_qdot       n_scene x nq       OUT configuration_derivative!
 *   d_H          n_scene x nv x nv  OUT mass_matrix!, the full symmetric matrix, row-major
 *   d_c          n_scene x nv       OUT dynamics_bias!: H vdot + c = tau + f
 * Any OUT pointer may be NULL: it is not written and the work it alone needs is not done (d_qdot reads d_q and d_v only; d_H reads
 * d_x_w_b only; d_c reads d_x_w_b, d_twist_w_b and d_v; PFC_ERR_BAD_ARG if an input an output needs is NULL).  The arithmetic is plain
 * Float64 without fma, `x` the 3-vector cross product (a x b)_0 = a1 b2 - a2 b1 and cyclic, every 3-term dot product summed left to
 * right, dot6(a, b) = ((((a0 b0 + a1 b1) + a2 b2) + a3 b3) + a4 b4) + a5 b5; motion vectors and wrenches are [angular; linear] in
 * world about the world origin:
 *   qdot.  revolute, prismatic: v.  floating, q = [p; t], v = [w; u] in the frame after: p2 = (p0 p0 + p1 p1) + p2 p2,
 *     pw = (p0 w0 + p1 w1) + p2 w2;  pdot_r = 0.25 (((1 - p2) w_r + 2 (p x w)_r) + (2 pw) p_r);  tdot_r = (R_r0 u0 + R_r1 u1) + R_r2 u2
 *     with R the joint rotation R_j(p) of pfc_kinematics_device.
 *   world inertia of body b, pose (R, t), record (M, cp, m): hc_r = (R_r0 cp0 + R_r1 cp1) + R_r2 cp2;  mt_r = m t_r;  h_r = hc_r + mt_r;
 *     B_rc = (R_r0 M_0c + R_r1 M_1c) + R_r2 M_2c;  A_rc = (B_r0 R_c0 + B_r1 R_c1) + B_r2 R_c2;  s1 = (t0 hc0 + t1 hc1) + t2 hc2;
 *     s2 = (t0 mt0 + t1 mt1) + t2 mt2;  for r <= c: J_rc = (A_rc - (hc_r t_c + t_r hc_c)) - mt_r t_c, on the diagonal + (2 s1 + s2)
 *     added last;  J_cr = J_rc.  I_b = (J, h, m), added componentwise.
 *   I [w; u] = [((J_r0 w0 + J_r1 w1) + J_r2 w2) + (h x u)_r;  m u_r - (h x w)_r]
 *   a x_m b = [a_w x b_w;  (a_w x b_u) + (a_u x b_w)]        a x* f = [(a_w x f_n) + (a_u x f_f);  a_w x f_f]
 *   the columns S_i of pfc_kinematics_device, formed again from d_x_w_b (the same bytes; the handle's column buffer is not read)
 *   composite inertia Ic_b = I_b + I_d1 + I_d2 + ... over b's descendants in increasing body order, summed left to right
 *   H[i,j] for j <= i, b = the body whose joint owns i: dot6(S_j, Ic_b S_i) if j's joint lies on the root -> b path, +0.0 otherwise;
 *     H[j,i] is a copy of H[i,j].
 *   joint twist jt_b = (S_i0 v_i0 + S_i1 v_i1) + ... over the joint's coordinates (fixed: +0.0 six times)
 *   a_b = a_parent + (tw_b x_m jt_b) elementwise, from a_world = [+0.0 (3); -g], tw_b = d_twist_w_b's row
 *   w_b = I_b a_b + (tw_b x* (I_b tw_b)) elementwise;  W_b = w_b + w_d1 + w_d2 + ... as the composite inertia;  c_i = dot6(S_i, W_b)
 * -- the same bytes on every call, handle and entry point; no atomics.  The call is NOT an evaluation: a kept value pass, Dual reuse,
 * pfc_check and pfc_last_* are as they were.  n_scene = 0 is a no-op.  PFC_ERR_STATE before pfc_set_inertia; PFC_ERR_BAD_ARG if
 * 44 n_body + 12.5 nv doubles exceed 64 KiB (the scene's tables live in LDS).  Multi-device handles: the first device.
 */
int pfc_dynamics_device(pfc_handle h, int n_scene, const double *d_q, const double *d_v, const double *d_x_w_b, const double *d_twist_w_b,
                        double *d_qdot, double *d_H, double *d_c, void *stream);
/* The same with host buffers, synchronous: the same kernel, the same bytes. */
int pfc_dynamics(pfc_handle h, int n_scene, const double *q, const double *v, const double *x_w_b, const double *twist_w_b,
                 double *qdot, double *H, double *c);

/*
 * vdot = H^-1 ((f - c) + tau): sum_all_forces!, cholesky! and ldiv!.  One kernel, one workgroup per scene with L in LDS, enqueued on
 * `stream`:
 *   d_H, d_c   pfc_dynamics_device's outputs (the lower triangle of H is read)      d_f  n_scene x nv, f_generalized
 *   d_tau      n_scene x nv, or NULL: zeros (a controller's or any other generalized force)
 *   d_vdot     n_scene x nv  OUT            d_info  n_scene OUT, or NULL
 * The mechanism's nv must not exceed PFC_MAX_NV_SOLVE (one lane per row, L of 64 x 64 doubles = 32 KiB of LDS): PFC_ERR_BAD_ARG
 * before anything is launched.  LAPACK's bits are not reproduced; the order is this, in plain Float64 without fma, sqrt and /
 * correctly rounded:
 *   rhs_i = (f_i - c_i) + tau_i  (tau NULL: + 0.0)
 *   for j ascending: s_ij = ((H_ij - L_i0 L_j0) - L_i1 L_j1) - ... - L_i,j-1 L_j,j-1 for i >= j;  L_jj = sqrt(s_jj);  L_ij = s_ij / L_jj
 *   y_i = (((rhs_i - L_i0 y_0) - L_i1 y_1) - ... - L_i,i-1 y_i-1) / L_ii, i ascending
 *   vdot_i = (((y_i - L_n-1,i vdot_n-1) - L_n-2,i vdot_n-2) - ... - L_i+1,i vdot_i+1) / L_ii, i descending
 * If a pivot s_jj is not > 0 (NaN included) the scene's whole vdot is NaN and d_info[scene] = j + 1; otherwise d_info[scene] = 0.
 * That is a per-scene numeric flag, not an error state: other scenes are unaffected and pfc_check is not involved.  Not an
 * evaluation; n_scene = 0 is a no-op; PFC_ERR_STATE before pfc_set_mechanism (the inertias are not needed).
 */
#define PFC_MAX_NV_SOLVE 64
int pfc_accelerations_device(pfc_handle h, int n_scene, const double *d_H, const double *d_c, const double *d_f, const double *d_tau,
                             double *d_vdot, int *d_info, void *stream);
/* The same with host buffers, synchronous: the same kernel, the same bytes. */
int pfc_accelerations(pfc_handle h, int n_scene, const double *H, const double *c, const double *f, const double *tau, double *vdot,
                      int *info);

/*
 * Exactly pfc_eval_state_device with d_f required, then pfc_dynamics_device, then pfc_accelerations_device, on one stream: from
 * x = [q; v; s] to qdot, vdot and sdot (which stays in d_sdot's rows; the host lays out xx).  All buffers are the caller's; required
 * are those pfc_eval_state_device requires with d_f, and d_qdot, d_H, d_c, d_vdot; d_tau and d_info may be NULL.  Everything the parts
 * would refuse -- missing inertias and the nv cap included -- is checked before the first launch.  pfc_check() afterwards as after
 * pfc_eval_device; on PFC_ERR_OVERFLOW the outputs are undefined and the call is re-issued.
 */
int pfc_state_derivative_device(pfc_handle h, int n_items, const int *d_ins_ids, const int *d_scene, int n_scene,
                                const double *d_q, const double *d_v, const double *d_s, const double *d_tau,
                                double *d_x_w_b, double *d_twist_w_b, double *d_jac,
                                double *d_pose, double *d_twist, double *d_x_w_r2, int *d_body_1, int *d_body_2,
                                double *d_wrench, double *d_sdot, int *d_counts, double *d_f,
                                double *d_qdot, double *d_H, double *d_c, double *d_vdot, int *d_info, void *stream);
/* The host-buffer form: pfc_eval_state, pfc_dynamics, pfc_accelerations.  Optional are pfc_eval_state's optional arguments but f, and
 * tau and info.  Synchronous. */
int pfc_state_derivative(pfc_handle h, int n_items, const int *ins_ids, const int *scene, int n_scene,
                         const double *q, const double *v, const double *s, const double *tau,
                         double *x_w_b, double *twist_w_b, double *jac,
                         double *pose, double *twist, double *x_w_r2, int *body_1, int *body_2,
                         double *wrench, double *sdot, int *counts, double *f,
                         double *qdot, double *H, double *c, double *vdot, int *info);

/*
 * Dual kinematics from joint states: the partials of the bodies' world poses, twists and geometric Jacobians that RigidBodyDynamics
 * gives the reference on the Dual state of a Jacobian chunk (src/radau/radau_functions.jl:2-14), formed on the device from (q, v) and
 * the chunk's seed directions -- the front of the chain state + seeds -> body-state partials -> item seeds ->
 * pfc_eval_dual_device[_more] -> pfc_scatter_generalized_dual_device.  Two kernels enqueued on `stream` (NULL = the handle's own)
 * without a host synchronisation, for n_dir (1..16, else PFC_ERR_BAD_ARG) seed directions:
 *   d_q, d_v      the values, as pfc_kinematics_device (d_v may be NULL only when d_dtwist_w_b is: PFC_ERR_BAD_ARG otherwise)
 *   d_dq          n_scene x n_dir x nq   partials of q, direction dir of scene s at row s n_dir + dir
 *   d_dv          n_scene x n_dir x nv   partials of v, likewise
 *                 each may be NULL: zeros, the same bytes as an array of zeros (the chunk that seeds only velocities or only
 *                 configurations)
 *   d_dx_w_b      n_scene n_body x n_dir x 12      OUT partials of x_w_b, pfc_dual_seeds_from_bodies_device's d_dx_w_b: direction dir of
 *                 body b of scene s at row (s n_body + b) n_dir + dir
 *   d_dtwist_w_b  n_scene n_body x n_dir x 6       OUT partials of twist_w_b, its d_dtwist_w_b
 *   d_djac        n_scene n_body x n_dir x nv x 6  OUT partials of the Jacobians, pfc_scatter_generalized_dual_device's d_djac for the
 *                 scene-offset body ids pfc_items_from_bodies_device writes: column c at row ((s n_body + b) n_dir + dir) nv + c
 * Any OUT pointer may be NULL: it is not written, and the work it alone needs is not launched.  The arithmetic is the statement of
 * pfc_kinematics_device run on (value, partial) numbers with ForwardDiff's rules, without fma and with nothing restated:
 *   sums and differences componentwise;  d(a b) = da b + a db;  a literal or a mechanism constant (x_p_j, an axis) is {x, 0.0};
 *   a / b = {a.v / b.v, a.d (1.0 / b.v) + b.d (-(a.v / (b.v b.v)))};
 *   sin th = {sin th.v, cos th.v th.d},  cos th = {cos th.v, -(sin th.v th.d)}, the values being those of pfc_kinematics_device.
 * There is no shortcut for a zero seed: a direction that seeds none of a body's ancestors goes through the same expressions, and
 * its partials are the signed zeros of that arithmetic.  The partial columns of a body's non-ancestors are +0.0 six times.  The value
 * parts are pfc_kinematics_device's bytes and are not stored.  The same bytes on every call, handle and entry point.  The call is NOT
 * an evaluation: a kept value pass, Dual reuse, pfc_check and pfc_last_* are as they were (a pfc_eval_dual_device_more may still
 * follow the evaluation before it).  n_scene = 0 is a no-op.  PFC_ERR_STATE before pfc_set_mechanism; nothing is written where the
 * call is refused.  The call keeps the partial columns in a handle buffer that grows on demand only: calls on different streams must
 * be ordered by the caller.  Multi-device handles: the first device.
 */
int pfc_kinematics_dual_device(pfc_handle h, int n_scene, int n_dir, const double *d_q, const double *d_v,
                               const double *d_dq, const double *d_dv,
                               double *d_dx_w_b, double *d_dtwist_w_b, double *d_djac, void *stream);
/* The same with host buffers, synchronous: the same kernels, the same bytes. */
int pfc_kinematics_dual(pfc_handle h, int n_scene, int n_dir, const double *q, const double *v, const double *dq, const double *dv,
                        double *dx_w_b, double *dtwist_w_b, double *djac);

/*
 * The Dual sibling of pfc_eval_state_device.  On one stream, with n_body and nv of the mechanism: pfc_kinematics_device,
 * pfc_kinematics_dual_device, exactly pfc_eval_dual_bodies_device, then pfc_scatter_generalized_dual_device with accumulate = 0 into
 * d_f (n_scene x nv) and d_df (n_scene x n_dir x nv): (q, v) and their seed directions in, f_generalized and its partials out, with no
 * upload per chunk but the seeds.  d_df = NULL skips the scatter; d_f may be NULL even with d_df given (partials only).  All buffers are
 * the caller's and all are required but d_ins_ids, d_scene, d_s, d_ds, d_dq, d_dv, d_counts (as in the parts), d_f and d_df; with
 * d_df also d_jac, d_djac, d_x_w_r2, d_dx_w_r2, d_body_1 and d_body_2 (without it each of these may be NULL: not written).
 * pfc_check() afterwards as after pfc_eval_dual_device; on PFC_ERR_OVERFLOW the outputs are undefined and the call is re-issued
 * (everything is formed again, to the same bytes).  States and errors are those of the parts, checked before anything is launched;
 * PFC_ERR_BAD_ARG if an instruction the items use is bound to a body >= n_body of the mechanism.  There is no accumulate variant: a
 * host that accumulates calls the parts.
 */
int pfc_eval_dual_state_device(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene,
                               const double *d_q, const double *d_v, const double *d_dq, const double *d_dv,
                               const double *d_s, const double *d_ds,
                               double *d_x_w_b, double *d_twist_w_b, double *d_jac,
                               double *d_dx_w_b, double *d_dtwist_w_b, double *d_djac,
                               double *d_pose, double *d_twist, double *d_x_w_r2, int *d_body_1, int *d_body_2,
                               double *d_dpose, double *d_dtwist, double *d_dx_w_r2,
                               double *d_wrench, double *d_sdot, double *d_dwrench, double *d_dsdot, int *d_counts,
                               double *d_f, double *d_df, void *stream);
/*
 * The later chunks of a Jacobian at the kept point, from the seeds of (q, v): pfc_kinematics_dual_device, then exactly
 * pfc_eval_dual_bodies_device_more, then the Dual scatter into d_df (NULL: no scatter).  It reads the value buffers the first chunk
 * left -- d_x_w_b, d_twist_w_b, d_jac, d_x_w_r2, d_body_1, d_body_2 and d_wrench (the last five with d_df only) -- and writes only
 * partials: no value output, no f.  Single-device handles check _more's preconditions before anything is launched --
 * PFC_ERR_STATE without a checked pfc_eval_dual_device evaluation to extend, PFC_ERR_BAD_ARG if n_items is not that evaluation's -- and
 * then write nothing.  Multi-device handles form the kinematics partials and the seeds on the first device and then return _more's own
 * status, as pfc_eval_dual_bodies_device_more documents.  Follow with pfc_check() as after pfc_eval_dual_device_more.
 */
int pfc_eval_dual_state_device_more(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene,
                                    const double *d_q, const double *d_v, const double *d_dq, const double *d_dv, const double *d_ds,
                                    const double *d_x_w_b, const double *d_twist_w_b, const double *d_jac,
                                    double *d_dx_w_b, double *d_dtwist_w_b, double *d_djac,
                                    const double *d_x_w_r2, const int *d_body_1, const int *d_body_2, const double *d_wrench,
                                    double *d_dpose, double *d_dtwist, double *d_dx_w_r2, double *d_dwrench, double *d_dsdot,
                                    double *d_df, void *stream);

/*
 * Dual forward dynamics from joint states: the partials of qdot, H, c and vdot that the Dual method of calcXd! gets from
 * RigidBodyDynamics on the Dual state of a Jacobian chunk (src/radau/radau_functions.jl:2-14), so that one call per chunk yields a
 * column block of d[qdot; vdot; sdot] / d[q; v; s] with no upload but the seed directions.
 *
 * pfc_dynamics_dual_device: one kernel (one 64-lane workgroup per (scene, direction), its tables in LDS) enqueued on `stream`
 * (NULL = the handle's own) without a host synchronisation, for n_dir (1..16, else PFC_ERR_BAD_ARG) seed directions:
 *   d_q, d_v, d_dq, d_dv        as pfc_kinematics_dual_device (d_dq / d_dv NULL: zeros, the same bytes as an array of zeros)
 *   d_x_w_b, d_twist_w_b        pfc_kinematics_device's outputs for the same (q, v)
 *   d_dx_w_b, d_dtwist_w_b      pfc_kinematics_dual_device's outputs for the same (q, v) and seeds, in its layout
 *   d_dqdot      n_scene x n_dir x nq       OUT partials of qdot, direction dir of scene s at row s n_dir + dir
 *   d_dH         n_scene x n_dir x nv x nv  OUT partials of H, the full matrix, row-major, the mirror a copy
 *   d_dc         n_scene x n_dir x nv       OUT partials of c
 * Any OUT pointer may be NULL: it is not written and its stages are skipped.  An input an output needs must not be NULL
 * (PFC_ERR_BAD_ARG): d_dqdot needs d_q and d_v; d_dH needs d_x_w_b and d_dx_w_b; d_dc needs d_x_w_b, d_twist_w_b, d_dx_w_b,
 * d_dtwist_w_b and d_v.  The arithmetic is the statement of pfc_dynamics_device run on (value, one partial) numbers with the rules
 * pfc_kinematics_dual_device states, without fma and with nothing restated: gravity, the inertia records, the axes and the literals
 * are {x, 0.0} (a_world = [{+0.0, +0.0} (3); -{g, 0.0}]); the poses and twists are {d_x_w_b, d_dx_w_b} and {d_twist_w_b,
 * d_dtwist_w_b}, q and v are {q, dq} and {v, dv}.  Revolute and prismatic joints: dqdot = dv; floating joints: the qdot statement on
 * {q, dq}, {v, dv}, the joint rotation through the quotient rule.  dH[i,j] is +0.0 where j's joint is not on the root -> body(i)
 * path.  There is no shortcut for zero seeds.  The value parts are pfc_dynamics_device's bytes and are not stored.  The same bytes on
 * every call, handle and entry point; no atomics.  The Dual tables are twice the value tables: PFC_ERR_BAD_ARG, before anything is
 * launched and with nothing written, if 88 n_body + 24.5 nv doubles exceed 64 KiB (the value call for the same mechanism may still
 * pass; a 64-link chain takes 57.6 kB).  PFC_ERR_STATE before pfc_set_inertia.  The call is NOT an evaluation: a kept value pass, Dual
 * reuse, pfc_check and pfc_last_* are as they were.  n_scene = 0 is a no-op.  Multi-device handles: the first device.
 */
int pfc_dynamics_dual_device(pfc_handle h, int n_scene, int n_dir, const double *d_q, const double *d_v, const double *d_dq,
                             const double *d_dv, const double *d_x_w_b, const double *d_twist_w_b, const double *d_dx_w_b,
                             const double *d_dtwist_w_b, double *d_dqdot, double *d_dH, double *d_dc, void *stream);
/* The same with host buffers, synchronous: the same kernel, the same bytes. */
int pfc_dynamics_dual(pfc_handle h, int n_scene, int n_dir, const double *q, const double *v, const double *dq, const double *dv,
                      const double *x_w_b, const double *twist_w_b, const double *dx_w_b, const double *dtwist_w_b,
                      double *dqdot, double *dH, double *dc);

/*
 * vdot and its partials: the exact derivative of the solve, dvdot = H^-1 (d rhs - dH vdot), with the value factor -- not the
 * factorisation run on (value, partial) numbers, from which it differs by rounding of order kappa(H) eps.  One kernel, one 64-lane
 * workgroup per scene, lane = row, enqueued on `stream`:
 *   d_H, d_c, d_f, d_tau   as pfc_accelerations_device
 *   d_dH, d_dc             pfc_dynamics_dual_device's outputs       d_df  n_scene x n_dir x nv, pfc_eval_dual_state_device's d_df
 *   d_dtau                 n_scene x n_dir x nv, or NULL: zeros
 *   d_vdot   n_scene x nv          OUT, or NULL: pfc_accelerations_device's bytes
 *   d_dvdot  n_scene x n_dir x nv  OUT       d_info  n_scene OUT, or NULL: as pfc_accelerations_device
 * The order, in plain Float64 without fma: L, y and vdot as pfc_accelerations_device states; then per direction
 *   t_i = ((dH_i0 vdot_0 + dH_i1 vdot_1) + ...) + dH_i,n-1 vdot_n-1, j ascending
 *   r_i = ((df_i - dc_i) + dtau_i) - t_i  (dtau NULL: + 0.0)
 * and dvdot from r by the same two substitutions with the same L (the directions run together: each lane carries n_dir
 * accumulators, so the number of sequential steps does not grow with n_dir).  A pivot that is not > 0 makes the scene's vdot and all
 * its dvdot NaN and sets d_info[scene] = j + 1.  n_dir in 1..16 and nv <= PFC_MAX_NV_SOLVE, else PFC_ERR_BAD_ARG before anything is
 * launched.  LDS: L and (1 + N) nv doubles, N = n_dir rounded up to 1, 2, 4, 8 or 16 (a lane's accumulators; the slots beyond n_dir
 * repeat the last direction and are not stored), 41.5 kB at the cap.  Not an evaluation; n_scene = 0 is a no-op; PFC_ERR_STATE before
 * pfc_set_mechanism.
 */
int pfc_accelerations_dual_device(pfc_handle h, int n_scene, int n_dir, const double *d_H, const double *d_c, const double *d_f,
                                  const double *d_tau, const double *d_dH, const double *d_dc, const double *d_df, const double *d_dtau,
                                  double *d_vdot, double *d_dvdot, int *d_info, void *stream);
/* The same with host buffers, synchronous: the same kernel, the same bytes. */
int pfc_accelerations_dual(pfc_handle h, int n_scene, int n_dir, const double *H, const double *c, const double *f, const double *tau,
                           const double *dH, const double *dc, const double *df, const double *dtau, double *vdot, double *dvdot,
                           int *info);

/*
 * Exactly pfc_eval_dual_state_device with d_f and d_df required, then pfc_dynamics_device, pfc_dynamics_dual_device and
 * pfc_accelerations_dual_device, on one stream: three launches more than the Dual evaluation (k_accel is not launched).  d_tau and
 * d_dtau may be NULL (zeros), d_info may be NULL; d_qdot, d_H, d_c, d_vdot, d_dqdot, d_dH, d_dc and d_dvdot are required.  Everything
 * a part would refuse -- missing inertias, the nv cap, the Dual LDS limit and n_dir included -- is checked before the first launch,
 * and then nothing is written.  pfc_check() afterwards as after pfc_eval_dual_device.  There is no host-buffer form.
 */
int pfc_state_derivative_dual_device(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene,
                                     const double *d_q, const double *d_v, const double *d_dq, const double *d_dv,
                                     const double *d_s, const double *d_ds, const double *d_tau, const double *d_dtau,
                                     double *d_x_w_b, double *d_twist_w_b, double *d_jac,
                                     double *d_dx_w_b, double *d_dtwist_w_b, double *d_djac,
                                     double *d_pose, double *d_twist, double *d_x_w_r2, int *d_body_1, int *d_body_2,
                                     double *d_dpose, double *d_dtwist, double *d_dx_w_r2,
                                     double *d_wrench, double *d_sdot, double *d_dwrench, double *d_dsdot, int *d_counts,
                                     double *d_f, double *d_df,
                                     double *d_qdot, double *d_H, double *d_c, double *d_vdot, int *d_info,
                                     double *d_dqdot, double *d_dH, double *d_dc, double *d_dvdot, void *stream);
/*
 * The later chunks at the kept point: exactly pfc_eval_dual_state_device_more with d_df required, then pfc_dynamics_dual_device,
 * then pfc_accelerations_dual_device with d_vdot = NULL.  It reads d_H, d_c, d_f and d_tau as the first chunk left them and writes
 * only partials.  Checks and pfc_check() as above and as pfc_eval_dual_state_device_more.
 */
int pfc_state_derivative_dual_device_more(pfc_handle h, int n_items, int n_dir, const int *d_ins_ids, const int *d_scene, int n_scene,
                                          const double *d_q, const double *d_v, const double *d_dq, const double *d_dv, const double *d_ds,
                                          const double *d_tau, const double *d_dtau,
                                          const double *d_x_w_b, const double *d_twist_w_b, const double *d_jac,
                                          double *d_dx_w_b, double *d_dtwist_w_b, double *d_djac,
                                          const double *d_x_w_r2, const int *d_body_1, const int *d_body_2, const double *d_wrench,
                                          double *d_dpose, double *d_dtwist, double *d_dx_w_r2, double *d_dwrench, double *d_dsdot,
                                          double *d_df, const double *d_H, const double *d_c, const double *d_f,
                                          double *d_dqdot, double *d_dH, double *d_dc, double *d_dvdot, void *stream);

/*
 * The contact surface of n_items items: per item what the reference's TractionCache holds after forceAllElasticIntersections!
 * (src/structs.jl; filled by src/contact_algorithms_non_friction.jl:217-265), the clipped polygons it was integrated over, and
 * normal_wrench / normal_wrench_cop (src/contact_algorithms_normal.jl:2-34) -- what test/test_normal.jl:31-41 and
 * test/test_friction.jl:251-256 read.  Inputs as pfc_eval (the pressure depends on the twist through the damping term
 * max(0, 1 + chi edot), non_friction.jl:251-265; not on s, not on the friction model).  Everything is in frame r2.
 *   poly_off   n_items + 1        OUT CSR: the polygons of item i are [poly_off[i], poly_off[i + 1])
 *   poly_idx   cap_poly x 3       OUT {element of mesh_1, element of mesh_2, vertex count 3..8}
 *   poly_xyz   cap_poly x 8 x 3   OUT the vertices; unused slots 0
 *   poly_trac  cap_poly + 1       OUT CSR: the traction points of polygon k are [poly_trac[k], poly_trac[k + 1])
 *   trac       cap_trac x 8       OUT n(3) r(3) dA p per traction point (pfc_debug_tractions' layout)
 *   summary    n_items x 11       OUT normal wrench about the r2 origin [ang 3; lin 3], cop 3, sum p dA, sum dA; an item without
 *                                     traction points gets zeros (the reference's cop would be 0/0 there)
 *   counts     n_items x 4        OUT as pfc_eval's (may be NULL)
 *   totals     2                  OUT polygons, traction points
 * Canonical order whatever the options ("fused", "team", "split_min", "fixed_order", "debug"): polygons of an item by ascending
 * (element of mesh_1, element of mesh_2), only pairs whose clip left 3 or more vertices; the points of a polygon in the reference's
 * fan and quadrature order, skipping fan triangles of zero area and points with p <= 0 (integrate_patch, fillTractionCache*).  The
 * summary is summed in that order as well: two calls on the same inputs return the same bytes in every output.  Traction points
 * are bit-identical to the ones pfc_eval integrates.
 * Capacity: if totals exceed cap_poly or cap_trac the call returns PFC_ERR_OVERFLOW after writing totals, poly_off, summary and
 * counts, and writes no byte of poly_idx, poly_xyz, poly_trac or trac: grow the buffers and call again.  Internal work-list
 * overflows are handled inside the call, as pfc_eval handles them.  n_items = 0 writes poly_off[0] = poly_trac[0] = 0 and zero
 * totals.  poly_idx / poly_xyz may be NULL when cap_poly = 0, trac when cap_trac = 0.
 * The call counts as an evaluation: pfc_eval_dual_device_more after it returns PFC_ERR_STATE and pfc_eval_dual's automatic reuse
 * does not reach across it.  It changes no option.  A multi-device handle runs the call on its first device, with the same
 * result, bit for bit, as a single-device handle.  The candidate order is that of option fixed_order and has its limits:
 * log2(items) + log2(elements of mesh_1) + log2(tets of mesh_2) <= 64 (PFC_ERR_BAD_ARG otherwise); an item with more than
 * 4 096 candidates switches the handle's surface calls to a sort of the whole list.  Host buffers, synchronous.
 */
int pfc_contact_surface(pfc_handle h, int n_items, const int *ins_ids, const double *pose, const double *twist, long long cap_poly,
                        long long cap_trac, long long *poly_off, int *poly_idx, double *poly_xyz, long long *poly_trac, double *trac,
                        double *summary, int *counts, long long *totals);
/* The same with every buffer in device memory, enqueued on `stream` (NULL = the handle's own) without a host synchronisation; then
 * pfc_check(): PFC_ERR_OVERFLOW means re-issue -- after growing the buffers if *d_totals exceeds a capacity (the outputs named
 * above are written then), else a work list has grown. */
int pfc_contact_surface_device(pfc_handle h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist,
                               long long cap_poly, long long cap_trac, long long *d_poly_off, int *d_poly_idx, double *d_poly_xyz,
                               long long *d_poly_trac, double *d_trac, double *d_summary, int *d_counts, long long *d_totals,
                               void *stream);

/*
 * The contact surface with its friction half: what pfc_contact_surface returns, plus per traction point the friction force that
 * traction() computes (src/contact_algorithms_friction.jl:12-48) and per item the friction wrench, the total wrench, ṡ and the
 * bristle patch state.  pose, twist, s and ins_ids as pfc_eval (s may be NULL when no item is bristle: zeros).  poly_off,
 * poly_idx, poly_xyz, poly_trac, trac, summary, counts and totals are byte-identical to what pfc_contact_surface returns for the
 * same (ins_ids, pose, twist): the same launches compute them.  Frame r2 throughout.
 *   fric          cap_trac x 4       OUT per point in trac order: T_c (3) = traction(...) (already times p dA), and the branch
 *                                        taken as a double: 0 the first (regularized |vel_t|^2 < v_c^2, bristle |T̄s|^2 < mu_s^2), 1 the other
 *   fric_summary  n_items x 20       OUT [0:6] total wrench about the r2 origin [ang; lin] (= summary[0:6] + fric_summary[6:12], one
 *                                        add per component: what pfc_eval returns, in this order of summation);
 *                                        [6:12] friction wrench about the r2 origin;
 *                                        [12:18] ṡ: -(1/tau) (K̄^{-1/2} S⁻¹ w_fric_cop + s) for a bristle item with points, -s/tau
 *                                        for one without, zeros for a regularized item (bristle_wrench_in_world, no_contact!);
 *                                        [18] sum p dA and [19] the number of the points that took the first branch
 *   stiff         n_items x 84       OUT (may be NULL) K (36, column-major, k̄ included; calc_patch_spatial_stiffness! about the
 *                                        cop of summary), K̄^{-1/2} (36), diag S⁻¹ (6), Δ² (6) (decompose_K!, :85-132): what
 *                                        pfc_debug_stiffness exposes; zeros for regularized items and items without points
 * Every per-item sum is a fixed function of the canonical candidate list (no grid, timing, option or handle enters, no
 * atomics): two calls on the same inputs return the same bytes in every output.  Capacity as pfc_contact_surface, extended: on
 * PFC_ERR_OVERFLOW the call writes totals, poly_off, summary, fric_summary, stiff and counts, and writes no byte of poly_idx,
 * poly_xyz, poly_trac, trac or fric -- cap_poly = cap_trac = 0 returns every per-item row and no per-point output.  fric may be
 * NULL when cap_trac = 0.  The key limit, the sort fallback, the end of Dual reuse and the multi-device rule are those of
 * pfc_contact_surface.  Host buffers, synchronous.
 */
int pfc_contact_surface_fric(pfc_handle h, int n_items, const int *ins_ids, const double *pose, const double *twist, const double *s,
                             long long cap_poly, long long cap_trac, long long *poly_off, int *poly_idx, double *poly_xyz,
                             long long *poly_trac, double *trac, double *fric, double *summary, double *fric_summary, double *stiff,
                             int *counts, long long *totals);
/* The same with every buffer in device memory, enqueued on `stream` (NULL = the handle's own) without a host synchronisation;
 * then pfc_check(), as after pfc_contact_surface_device. */
int pfc_contact_surface_fric_device(pfc_handle h, int n_items, const int *d_ins_ids, const double *d_pose, const double *d_twist,
                                    const double *d_s, long long cap_poly, long long cap_trac, long long *d_poly_off, int *d_poly_idx,
                                    double *d_poly_xyz, long long *d_poly_trac, double *d_trac, double *d_fric, double *d_summary,
                                    double *d_fric_summary, double *d_stiff, int *d_counts, long long *d_totals, void *stream);

/* Options: "debug" (1: keep per-pair clip counts and materialise traction points of every item so that the
 * pfc_debug_* calls work), "profile" (1: bracket each stage with HIP events), "max_levels" (0 = automatic),
 * "bfs_levels" (-1 = automatic: level-synchronous seed expansion only until there are >= 2048 seed pairs),
 * "graph" (1 = capture the launch sequence into a hipGraph per evaluation shape and replay it; default 1),
 * "no_filter" (1 = run the whole broadphase in the exact Float64 kernel instead of the Float32 filter + Float64
 * resolver; same candidate set, for A/B checks), "split_min" (default 1025; 0 = never: an evaluation of at least
 * this many items with ins_ids given is run as two concurrent halves on two streams with their own work lists, the
 * vector-ALU-bound broadphase of one half sharing the CUs with the latency-bound narrowphase of the other; results,
 * counters and stream ordering are those of the unsplit call; a SPARSE PILE -- at least 1 024 items over small or mid-sized
 * trees of which at most a quarter were in contact the last time the handle evaluated that many items -- runs as one launch
 * sequence with wider broadphase workgroups instead: pfc_last_parts() tells; the two streams of a handle are tested once for
 * running side by side -- environment PFC_NO_QUEUE_TEST=1 skips the test; pfc_eval writes the inputs of evaluations of up to 4 096
 * items straight into device memory when the device has a large PCIe BAR -- PFC_NO_BAR_INPUTS=1 keeps them in pinned host memory), "dual_reuse" (default 1: pfc_eval_dual compares the
 * value inputs of a call above the small-scene limits with those of the previous call and, if they are bitwise equal,
 * runs only the Dual passes on the previous call's value pass -- the chunks of one Jacobian), "clip_min" (default 384; 0 = never: a launch of at
 * least this many items runs the narrowphase as a clip-only kernel that keeps every clipped polygon, followed by the
 * integration over the compacted polygons; same results up to the order of the sums), "poison" (diagnostic, default 0: before every
 * evaluation the work lists are filled with entries whose item index is -1; the kernels never follow an item index
 * out of range but report it, PFC_ERR_STATE "a work-list slot was read before it was written"), "fused" (default 1:
 * an evaluation of <= 256 items over small trees runs as ONE kernel, one workgroup per item, instead of the batched
 * launch sequence -- the scene sizes Radau evaluates, src/radau/radau_functions.jl:2-14,64-70; same results; 0 = always
 * batched; the debug / profile options imply the batched path), "clip_queue" (default 1: the clip-only kernel of a
 * tri-tet launch queues the candidates that pass the trivial reject in its polygon ring and clips 64 of them at a time;
 * 0 = the lane-per-candidate clip rounds; same results bit for bit), "vertex_fields" (default 1: the bristle friction pass
 * over the kept polygons, k_fric, evaluates pressure, damping argument and bristle traction once per fan corner and combines
 * them per quadrature point -- they are affine in the point; 0 = re-derives them at every point as the counting kernels do;
 * counts identical, friction wrench equal to rounding: ~1e-15 relative; "debug" evaluations always use the per-point form, so that the
 * friction sums are formed at exactly the traction points pfc_debug_tractions returns; other values PFC_ERR_BAD_ARG), "bin_split"
 * (default 5: the queueing clip kernel -- "clip_queue" -- keeps the clipped polygons of fewer than this many vertices from the front
 * of a candidate chunk's slot range upward and the others from its back downward, so that the 64 polygons a wave of the
 * integration and friction passes holds have fans of like length; value evaluations without a Dual list and without "fixed_order"
 * only, and launches of at least 2^20 candidates only -- 512-candidate chunks, what the gain was measured on; every other path keeps
 * the dense fill; same counts and traction points, sums equal up to their order; 0 = dense fill everywhere, the behaviour before the
 * option existed; 3..9 allowed; -9..-3: the split |value| in launches of every size, for tests; other values PFC_ERR_BAD_ARG), "integ_spec"
 * (default 2: a scenario WITHOUT a regularized instruction integrates its kept polygons -- the pass after the clip-only kernel,
 * "clip_min" -- in a form of k_integ that does not carry the regularized-friction lane: 1 = that form at two waves per SIMD, 2 = the
 * same at three waves, which the registers the lane held make room for; 0 = always the general kernel.  The arithmetic and the order
 * of every sum are the general kernel's: under "fixed_order" the three values return the same bytes.  A scenario with any regularized
 * instruction runs the general kernel whatever the value; Dual value passes and "fixed_order" use the forms too; other values
 * PFC_ERR_BAD_ARG), "quad_const" (default 1: a scenario whose instructions ALL have quadrature rule 2 runs the bristle-only forms of
 * "integ_spec" and the per-corner friction pass of "vertex_fields" with the rule as a compile-time constant -- the same literals and
 * expressions, so the same bits; 0 = the kernels read the rule from the item; a scenario with a rule-1 instruction runs those whatever
 * the value; other values PFC_ERR_BAD_ARG), "team" (default 48, at most 48; 0 = never: an evaluation of a few
 * pairs too big for one workgroup -- BASELINE's single 9 680-tet x 5 120-triangle pair -- runs as ONE kernel with a team
 * of up to this many workgroups per item -- while a workgroup of the team has at most ~1 200 leaves of the pair to descend: up
 * to 16 poses of that pair; beyond that the batched path is faster --, and a few mid-sized items -- a 972-tet box on the
 * ground -- with a small team each (one workgroup per 128 leaves, at most 32); same results up to the order of the sums;
 * pfc_last_team().  Team-mates wait for
 * each other inside the launch: several handles evaluating such scenes at the same moment on one device may each get
 * only part of a team resident; the wait is bounded (~65 ms), the evaluation is then re-issued on the batched path.  Inside
 * one process that case does not arise: a device has one team slot, a handle that finds it taken evaluates without a team at
 * once), "team_fault" (diagnostic, default -1: this rank of every team behaves as if its wait for the team had timed out while
 * the others saw it arrive; the evaluation must come back re-issued on the batched path, never with a wrong result),
 * "multi_min" (multi-device handles, see pfc_create_multi), "fused_f32" (default 1: the one-launch kernel runs the batched
 * broadphase's single-precision SAT filter in front of the exact Float64 test, undecided pairs settled in the same iteration;
 * same node tests, candidates and results; 0 = exact test only; items whose pose has a frame axis parallel to one of the other
 * body's -- a box resting on a plane -- run with the filter off by themselves), "dual_fold" (default 1: pass B of a Dual evaluation of
 * tri-tet scenes is formed inside pass A), "fixed_order" (default 0.  1: BIT-REPRODUCIBLE evaluations.  The reference adds an
 * instruction's traction points in one order (src/contact_algorithms_non_friction.jl:136-143), so calcXd! gives the same bits
 * every time; the default path here appends candidates in the order its workgroups finish and sums with atomics, which changes
 * last bits from run to run -- and, where decompose_K! clamps an eigenvalue that is zero in exact arithmetic at 1e-16 sigma_max
 * (a flat patch; src/contact_algorithms_friction.jl:92), whole partials.  With the option on the candidate list is sorted by
 * (item, element of mesh_1, tet of mesh_2), every per-item sum of the value and Dual passes is added in list order, and the Dual
 * eigen-decomposition takes the value of K from the value pass: two evaluations of the same inputs on handles set up the same
 * way return the same bit patterns in wrench, sdot, every partial and every counter.  Batched path only while the option is on, whatever "fused", "team"
 * and "split_min" say (no one-launch kernel, no two-half split: a reference-sized scene costs 100 - 180 us instead of 35 - 90);
 * with "debug" the value pass's sums are the debug kernel's atomics again; costs a
 * radix sort of the candidate list's capacity per evaluation (BASELINE config 5: 0.29 -> 0.48 ms, an 8 192-pose batch 3.9 -> 5.4 ms).  Needs
 * log2(items) + log2(elements of mesh_1) + log2(tets of mesh_2) <= 64 (PFC_ERR_BAD_ARG otherwise) and at most 4 096 x 512
 * candidates per item (PFC_ERR_STATE)). */
int pfc_set_option(pfc_handle h, const char *name, long long value);

/* Totals of the last checked evaluation: out[0..7] = {node tests, candidate pairs, non-empty pairs, traction
 * points, broadphase levels launched, frontier peak, status word, n_items}. */
int pfc_get_stats(pfc_handle h, long long *out8);

/* Per-stage device time of the last evaluation in ms (profile option): out[0..5] = {setup, broadphase,
 * narrowphase, bristle passes (cop + K + eigen + friction), finalisation, total}.  Synchronises.  If the evaluation
 * ran as two concurrent halves (pfc_last_parts() == 2) a stage time is the mean over the two half-launches, each of
 * which processed half of the items while stages of the other half were running; total is the longer half. */
int pfc_get_stage_ms(pfc_handle h, float *out6);
int pfc_last_parts(pfc_handle h);   /* 1, or 2 if the last checked evaluation ran as two concurrent halves; 0: it ran as the
                                     * single fused small-scene kernel (option "fused") */
int pfc_last_team(pfc_handle h);    /* workgroups per item of the last checked evaluation if it ran as one fused kernel (1: a
                                     * workgroup per item; > 1: a team per item, option "team"), else 0 */
int pfc_last_dual_reused(pfc_handle h);   /* 1 if the last Dual evaluation ran only its Dual passes on the value pass of the
                                             previous one (pfc_eval_dual_device_more, or pfc_eval_dual with equal value inputs) */

/*
 * Debug views of the last evaluation (debug option), needed to restate test/test_normal.jl:31-41 and
 * test/test_friction.jl:228-236,251-256 which read m.float.bodyBodyCache.{TractionCache,spatialStiffness}:
 *   pfc_debug_pairs       candidate (i_1, i_2) pairs of an item (the TT_Cache contents, order unspecified) and the
 *                         vertex count of each clipped polygon; returns the number of pairs of that item
 *   pfc_debug_tractions   TractionCache entries of an item, 8 doubles each: n(3) r(3) dA p
 *   pfc_debug_stiffness   spatialStiffness of a bristle item: K, K̄^{-1/2} (column-major 6x6), S^{-1}, and the cop
 * Each returns a count (>= 0) or -(pfc_status); if the count exceeds cap only cap entries were written.
 */
int pfc_debug_pairs(pfc_handle h, int item, int *pairs, int *clip_n, int cap);
int pfc_debug_tractions(pfc_handle h, int item, double *buf, int cap);
int pfc_debug_stiffness(pfc_handle h, int item, double *K36, double *Kbar_inv_sqrt36, double *Sinv6, double *cop3);

/* Diagnostic builds only (-DPFC_STAMPS): cycles the waves spent per phase in the last evaluation; zeros otherwise.
 * out[0..5]  narrowphase {gather+transform, clip, slot reservation, integration, reductions, wave rounds}
 * out[8..12] broadphase  {pop + node loads, SAT, push + flush, iterations, node pairs tested} */
int pfc_debug_stamps(pfc_handle h, long long *out16);

/* Device arithmetic self-test: out[0..n) = x/y, out[n..2n) = sqrt(|x|), out[2n..3n) = fma(x, y, x) computed on the
 * GPU, so tests can check that device division / sqrt / fma are correctly rounded (bitwise = host). */
int pfc_selftest_math(pfc_handle h, int n, const double *x, const double *y, double *out3n);

/* Device self-test of the Dual path's eigen step: for n symmetric 6x6 K̄ (Kbar36) and directions dK̄ (dKbar36), column-major,
 * out72 per matrix = K̄^{-1/2} (36) then its Frechet derivative along dK̄ (36), by the code k_dual_eig runs (one wave per
 * matrix).  Vlam42 NULL: the device Jacobi diagonalises K̄; else per matrix the eigenvectors V (36, column-major) and the
 * eigenvalues (6) are taken from it, as with a stored decomposition (option fixed_order, PFC_DUAL_VALUE_K). */
int pfc_selftest_kis(pfc_handle h, int n, const double *Kbar36, const double *dKbar36, const double *Vlam42, double *out72);

/*
 * Parts of the Radau IIA step (csrc/pfc_radau.h): the reference's simplified-Newton integrator src/radau/ (updateInvC!, calcEw!,
 * updateStageX!, simple_newton!; radau_functions.jl:72-125, radau_solve.jl:47-99) for a batch of n_scene independent scenes of NX
 * states each, every scene with its own step size h and rule.  Rule 1 (one stage, implicit Euler) and rule 2 (three stages, order 5)
 * only; the reference's rules 3 - 6 are refused.  These are the parts on caller buffers and a caller stream (NULL: the handle's);
 * asynchronous.  They read nothing of the handle but its device and stream.
 * Arithmetic: plain Float64, no fma, in the written order below -- tests/test_radau_abi.py restates it in Python floats and
 * tests/test_gpu_radau.py compares bytes.  A "wave sum" of 64 numbers v[0..64) (entries >= NX are +0.0) is six rounds
 * v[i] <- v[i] + v[i ^ off], off = 32, 16, 8, 4, 2, 1.  Complex numbers are (re, im) pairs; (a + bi)(c + di) = (ac - bd) + (ad + bc)i,
 * (a + bi) / (c + di) = ((ac + bd) / (cc + dd)) + ((bc - ad) / (cc + dd))i.
 */
#define PFC_MAX_NX_RADAU 64   /* states per scene: one lane per state */

/* The compiled constants of a rule (generated by scripts/radau_tables.py from 50-digit arithmetic): *ns stages; c (ns), A (ns x ns, by
 * rows); lam (ns complex), T and Tinv (ns x ns complex, by rows) with A^-1 T = T diag(lam), unit-norm columns, lam[0] real and
 * lam[2] = conj(lam[1]); bhat (1 + ns): bhat0 = 1 / lam[0], then bhat.  Any output may be NULL.  PFC_ERR_BAD_ARG for a rule other
 * than 1 or 2. */
int pfc_radau_table(int rule, int *ns, double *c, double *A, double *lam, double *T, double *Tinv, double *bhat);

/* updateInvC! as factorisations instead of explicit inverses.  d_neg_J: n_scene x NX x NX, column-major (-J(i, j) of scene s at
 * (s NX + j) NX + i); d_h, d_rule: n_scene; d_active: n_scene or NULL -- a scene whose word is not 1 is left alone.  Per scene, with
 * hinv = 1 / h:  factor 0 = P0 (-J + (hinv lam_1) I), real;  factor 1, rule 2 only, = P1 (-J + (hinv lam_2) I), complex, the diagonal
 * (-J_kk + hinv Re lam_2, hinv Im lam_2).  The matrix of lam_3 is the conjugate of the second (J is real) and is not factored (the
 * reference inverts all three).  Right-looking LU, column k = 0 .. NX - 1: the pivot row p is the first row >= k of maximal
 * |re| + |im| (a NaN counts as +inf); rows k and p are exchanged; l_i = a_ik / a_kk, then a_ij <- a_ij - l_i a_kj, j = k + 1 .. NX - 1.
 * d_lu0 (n_scene x NX x NX) and d_lu1 (n_scene x NX x NX x 2) receive L (unit diagonal, not stored) and U over each other,
 * column-major; d_perm (n_scene x 2 x NX): row i of P A is row perm[i] of A; d_info (n_scene x 2): 0, or k + 1 at the first exactly
 * zero pivot, where the factorisation stops (columns < k final, the rest as reduced so far).  info of the absent factor 1 of a
 * rule-1 scene is 0; its lu1 and perm rows are not written.  One launch, 2 n_scene one-wave workgroups; each reserves the complex
 * factor's 16 NX^2 bytes of LDS (the real factor uses 8 NX^2 of them).  PFC_ERR_BAD_ARG: NX outside 1 .. PFC_MAX_NX_RADAU, null buffer. */
int pfc_radau_factor_device(pfc_handle h, int n_scene, int nx, const double *d_neg_J, const double *d_h, const int *d_rule,
                            const int *d_active, double *d_lu0, double *d_lu1, int *d_perm, int *d_info, void *stream);

/* One iteration of simple_newton! for every scene whose d_istate word 0 is 1; the other scenes are not touched.
 * The stage-scene of (stage s, scene) is s n_scene + scene, three stages whatever the rule.  F_s, the state derivative of stage-scene
 * s, is read in place: [d_qdot (3 n_scene x nq); d_vdot (3 n_scene x nv); rows br_items[0 .. n_br) (host array, increasing, < n_ips) of
 * d_sdot (3 n_scene n_ips x 6)], NX = nq + nv + 6 n_br.  d_x0: n_scene x NX; d_X: 3 n_scene x NX, the stage states, updated.
 * d_nstate (n_scene x 8) = {theta, theta of the iteration before, Psi_k, the residuals of the last two iterations (+inf at the start of
 * an attempt), this iteration's residual, the h of the last committed step, unused}; d_istate (n_scene x 8) = {iterating, k_iter (0 at
 * the start of an attempt), the attempt's exit flag (-1 while iterating), attempt open (1 from the arming to pfc_radau_finish_device),
 * attempts of this step, the step's exit flag, k_iter of the last attempt, the parked mark (0 unless pfc_radau_finish_end_device set it)}.  *d_count is set to the number of scenes still
 * iterating.  Per scene, NS = 1 or 3 stages:
 *   k_iter += 1; a nonzero info of a factor the rule uses: flag 4, done.
 *   r_s = ((X_s - x0) + (-h A[s,0]) F_0) + (-h A[s,1]) F_1 ...;  residual = ((0 + sum r_0 r_0) + sum r_1 r_1) + .. (wave sums);
 *   Ew_0 = ((0 + ((hinv lam_1) Tinv[0,0]) r_0) + ..;  Ew_1 likewise with the complex product (hinv lam_2) Tinv[1,s]       (calcEw!)
 *   w_0 = factor 0 \ Ew_0, w_1 = factor 1 \ Ew_1: b <- P b; y_k, k ascending: b_i <- b_i - l_ik y_k (i > k); x_k = b_k / u_kk,
 *   k descending: b_i <- b_i - u_ik x_k (i < k)
 *   dZ_s = T[s,0] w_0 + 2 (Re T[s,1] Re w_1 - Im T[s,1] Im w_1)   -- the reference adds the three products T[s,j] w_j and takes the
 *   real part; w_2 = conj(w_1), so this differs by rounding only
 *   stage by stage: 10 < max |dZ_s| -> flag 3, done (earlier stages stay updated, as in the reference); else X_s <- X_s - dZ_s
 *   residual < tol_newton -> flag 0, done (declared after the update is applied, as in the reference)
 *   theta, Psi_k: k_iter == 1: theta = sqrt(residual), Psi_k = theta; else theta' = theta, theta = sqrt(residual), Psi_k = sqrt(theta' theta)
 *   three residuals rising strictly -> flag 3; else k_iter == k_iter_max -> flag 1
 * d_F_save (3 n_scene x NX, or NULL) receives F_s of this iteration in d_X's layout: the derivative buffers are overwritten by the
 * next evaluation, in which a scene that has converged is evaluated at x0, and pfc_radau_finish_device needs F of the last iteration.
 * Deviations from the reference: a non-finite residual or dZ gives flag 3 at once and updates nothing (the reference iterates on
 * NaNs to its limit); a singular factor gives flag 4 (the reference's getri! would throw).  Exit flag 2 is never produced, as in
 * the reference.  PFC_ERR_BAD_ARG: NX, the layout sizes, the item list, tol_newton < 0, k_iter_max < 1, null buffer. */
int pfc_radau_newton_device(pfc_handle h, int n_scene, int nx, int nq, int nv, int n_ips, int n_br, const int *br_items,
                            const double *d_qdot, const double *d_vdot, const double *d_sdot, const double *d_x0, const double *d_h,
                            const int *d_rule, const double *d_lu0, const double *d_lu1, const int *d_perm, const int *d_info,
                            double tol_newton, int k_iter_max, double *d_X, double *d_F_save, double *d_nstate, int *d_istate,
                            int *d_count, void *stream);

/*
 * The step itself: solveRadau (radau_solve.jl:2-30) for a batch of n_scene scenes of the handle's mechanism, each with n_ips items
 * whose instructions are ins_ids[0 .. n_ips) (item i of scene s is global item s n_ips + i; every instruction bound with
 * pfc_set_instruction_bodies).  The integrator state -- x, t, h, rule, cooldown, the norms -- and the workspace of every call below
 * live in device memory owned by the handle and are freed with it.  The differential equation is pfc_state_derivative_device on the
 * 3 n_scene stage-scenes and pfc_state_derivative_dual_device[_more] on the n_scene scenes, called unchanged.
 * pfc_radau_configure: params = {h0, tol_a, tol_r, tol_newton, h_max, h_min} or NULL for the reference's defaults {1e-4, 1e-4, 1e-4,
 * 1e-16, 0.01, 1e-8}; the reference's other defaults are k_iter_max 15, max_rule 2 (utility.jl:10), n_chunk 6, cooldown 10.
 * NX = nq + nv + 6 (items of a scene whose instruction is bristle).  PFC_ERR_STATE before pfc_finalize, pfc_set_mechanism or
 * pfc_set_inertia; PFC_ERR_BAD_ARG, with a message, for NX > PFC_MAX_NX_RADAU, nv > PFC_MAX_NV_SOLVE, a mechanism beyond the Dual
 * dynamics' LDS limit, max_rule other than 1 or 2, n_chunk outside 1..16, an unknown instruction.  A second call replaces the first.
 */
int pfc_radau_configure(pfc_handle h, int n_scene, int n_ips, const int *ins_ids, const double *params, int k_iter_max, int max_rule,
                        int n_chunk, int cooldown);
/* NX, the bristle items per scene and their item indices (bristle_items: room for PFC_MAX_NX_RADAU / 6).  Any may be NULL. */
int pfc_radau_sizes(pfc_handle h, int *nx, int *n_bristle, int *bristle_items);
/* x (n_scene x NX, host) and t (n_scene, host; NULL: zeros) in; h, rule, cooldown, theta, Psi_k and the norms are reset to what the
 * reference's constructors give (h0, rule 1, the cooldown, -9999, 9999, -9999), and every scene is active again: no scene is retired
 * or parked, and an end set with pfc_radau_set_end is dropped with its trajectory (end times +inf, nothing recorded). */
int pfc_radau_set_state(pfc_handle h, const double *x, const double *t);
int pfc_radau_get_state(pfc_handle h, double *x, double *t);      /* either may be NULL */
/* After pfc_radau_set_state: a step size, rule (1 .. max_rule) and cooldown (>= 0) per scene (n_scene each, host; NULL: as it is)
 * in place of the reset values -- a restart from pfc_radau_rule_state's figures, or scenes that start at different h.
 * PFC_ERR_BAD_ARG, and nothing is changed, for an h that is not finite and > 0, a rule or a cooldown out of range. */
int pfc_radau_set_rule_state(pfc_handle h, const double *h_scene, const int *rule, const int *cooldown);
/* tau (n_scene x nv, host; NULL: zeros), held constant over a step; its partials are zero (a torque that varies inside a step, with
 * partials: pfc_radau_set_feedback below, which adds its law to this tau).  With a controller set
 * (pfc_radau_set_controller) the value of a scene lasts until the controller first fires for it: a fire overwrites all nv entries. */
int pfc_radau_set_tau(pfc_handle h, const double *tau);
/*
 * One step of every scene that is not retired; synchronous.  The Jacobian chunks (seed, pfc_state_derivative_dual_device then _more,
 * each followed by pfc_check and re-issued on PFC_ERR_OVERFLOW, the columns gathered), then per attempt the factors and the loop
 * unpack -> pfc_state_derivative_device -> pfc_check -> newton, one word read back per pass (the scenes still iterating), then finish;
 * attempts repeat for the scenes finish armed again.  Converged and retired scenes are still evaluated (the shape is fixed) and
 * ignored.  Per scene (each may be NULL): h_taken (0 where no step was taken), the exit flag (0; 5: "time step is too small,
 * something is wrong" -- x and t are unchanged and the scene stays retired until pfc_radau_set_state; 6: at or past its end, nothing
 * done -- see pfc_radau_set_end; attempts and h_taken are then 0), k_iter of the last attempt, the attempts.  Any other status of an evaluation or its pfc_check (a state that left the scene non-finite, say) is returned as it
 * is; the integrator state is then undefined until pfc_radau_set_state.  No dense output: every attempt starts from X = x0
 * (the reference's interpolate.jl is not built).  Multi-device handles use their first device.  Every scene that is neither retired
 * nor parked is stepped by every call; scenes stop one by one at the end times of pfc_radau_set_end, and while an end is set the
 * step records the trajectory as pfc_radau_integrate does.  n_scene and n_ips are limited at configure time so that
 * 3 n_scene max(n_ips, n_body) rows of 24 words are indexed in int.
 */
int pfc_radau_step(pfc_handle h, double *h_taken, int *flags, int *iters, int *attempts);
/*
 * Integration to per-scene end times with the trajectory kept on the device: the loop of integrate_scenario_radau
 * (src/example_integrator.jl) for every scene of the batch.  After pfc_radau_set_state (PFC_ERR_STATE before it or before
 * pfc_radau_configure).
 * pfc_radau_set_end: t_final (n_scene, host; NULL: +inf, which never stops a scene) and the row budget max_rows of each scene (the
 * reference's max_steps + 1; 0: nothing is recorded).  Row 0 of a scene's trajectory becomes its (t, x) now, and no scene is parked
 * any more.  From then on every committed step of a scene appends the row (t, x) -- x after principal_value!, as the reference stores
 * it -- and the scene PARKS at the commit that leaves t_final < t (strict, as the reference's loop; a scene already past its end
 * still takes one step: the reference steps first and tests afterwards) or that fills its last row.  That step's exit flag is 0.  A
 * failed attempt and a retirement (flag 5) append nothing.  A parked scene is treated as a retired one: it is not armed, it is
 * evaluated at its committed x (the evaluation shape stays 3 n_scene) and its x, t, h, rule, cooldown and norms stay byte for byte;
 * pfc_radau_step reports exit flag 6 for it.  Parking ends with pfc_radau_set_state or the next pfc_radau_set_end.  The trajectory,
 * n_scene x max_rows x (1 + NX) doubles, is device memory owned by the handle: freed by the next pfc_radau_set_end,
 * pfc_radau_configure, pfc_radau_set_state and with the handle.  PFC_ERR_BAD_ARG, with a message and nothing changed: a NaN t_final,
 * max_rows < 0 or max_rows = 1.  PFC_ERR_NOMEM if the trajectory cannot be allocated: the previous end stays in force.
 * pfc_radau_integrate: batch steps -- pfc_radau_step's, parking and recording as above (with no end set: end times +inf, nothing
 * recorded) -- until no scene is live (neither retired nor parked) or max_steps (>= 0) steps were taken; *steps_done and *n_live (either
 * may be NULL) are the batch steps taken and the scenes live afterwards.  Per batch step the host reads one word per Newton pass and
 * two per finish (the scenes armed again; the scenes live); neither the records nor x are copied.  tau stays what pfc_radau_set_tau
 * set unless pfc_radau_set_controller gave a controller (below), which then runs at the top of every batch step on the device; a
 * caller with any other control law integrates one batch step at a time.
 * pfc_radau_trajectory_rows: the rows written per scene (n_scene ints, host).  pfc_radau_trajectory: rows [row0, row0 + n) of a scene
 * into t (n) and x (n x NX) (host; either may be NULL); PFC_ERR_BAD_ARG, nothing written, for a scene or a range outside what was
 * recorded; PFC_ERR_STATE for either call before pfc_radau_set_end.
 */
int pfc_radau_set_end(pfc_handle h, const double *t_final, int max_rows);
int pfc_radau_integrate(pfc_handle h, int max_steps, int *steps_done, int *n_live);
int pfc_radau_trajectory_rows(pfc_handle h, int *rows);
int pfc_radau_trajectory(pfc_handle h, int scene, int row0, int n, double *t, double *x);
/* Per scene 7 doubles: h, rule, cooldown, theta, Psi_k, x_err_norm, x_err_norm k+1. */
int pfc_radau_rule_state(pfc_handle h, double *out7);

/* The state layout the other parts share (nx, nq, nv, n_ips, n_br, br_items as above): scene s holds x = [q (nq); v (nv); 6 states per
 * bristle item], the reference's copyto! (src/extensions.jl:21-51); the items are uniform across scenes, item i of scene s is global
 * item s n_ips + i.  Chunk k of n_chunk-wide (1..16) chunks covers the states [k n_chunk, min((k + 1) n_chunk, NX)): direction d is
 * state k n_chunk + d, and the last chunk has fewer directions (n_dir).
 *
 * seed_indices! (radau_functions.jl:16-26): every entry of d_dq (n_scene x n_dir x nq), d_dv (n_scene x n_dir x nv) and d_ds
 * (n_scene n_ips x n_dir x 6) -- pfc_state_derivative_dual_device's seed layouts -- is written: 1.0 where the entry is the state its
 * direction seeds, +0.0 elsewhere (the s rows of items that are not bristle included). */
int pfc_radau_seed_device(pfc_handle h, int n_scene, int nx, int nq, int nv, int n_ips, int n_br, const int *br_items, int chunk,
                          int n_chunk, double *d_dq, double *d_dv, double *d_ds, void *stream);

/* write_indices! (radau_functions.jl:28-40): columns k n_chunk + d of d_neg_J (pfc_radau_factor_device's layout) = -[dqdot; dvdot; the
 * bristle rows of dsdot] of direction d, from pfc_state_derivative_dual_device[_more]'s outputs d_dqdot (n_scene x n_dir x nq), d_dvdot
 * (n_scene x n_dir x nv), d_dsdot (n_scene n_ips x n_dir x 6).  Chunk 0 also writes d_xdot0 (n_scene x NX) = [qdot; vdot; sdot] of the
 * value buffers (the reference's xx_0; they are not read for the later chunks and may be NULL there) and, where d_nstate and d_istate
 * are given, arms every scene whose step exit flag is not 5 and whose parked mark (the last word of its integer record; 0 unless
 * pfc_radau_finish_end_device set it) is 0 for the first attempt of a step: iterating = 1, k_iter = 0, attempt flag -1, attempt open,
 * attempts = 1, both remembered residuals +inf.  A parked scene whose flag is not 5 gets step exit flag 6 and attempts 0 instead. */
int pfc_radau_jacobian_device(pfc_handle h, int n_scene, int nx, int nq, int nv, int n_ips, int n_br, const int *br_items, int chunk,
                              int n_chunk, const double *d_dqdot, const double *d_dvdot, const double *d_dsdot, const double *d_qdot,
                              const double *d_vdot, const double *d_sdot, double *d_neg_J, double *d_xdot0, double *d_nstate,
                              int *d_istate, void *stream);

/* The stage states into the inputs of pfc_state_derivative_device on the 3 n_scene stage-scenes: d_q (3 n_scene x nq), d_v (.. x nv),
 * d_s (3 n_scene n_ips x 6; the rows of items that are not bristle are +0.0).  The evaluation shape is 3 n_scene whatever the rules, so
 * that a captured evaluation graph is reused: the unused stages of a rule-1 scene carry copies of its stage 0 and their derivatives
 * are ignored (two wasted scene evaluations per iteration of such a scene), and a scene that is not iterating is evaluated at d_x0
 * and ignored.  A scene at the start of an attempt (k_iter = 0) gets initialize_X_with_X0!: its three rows of d_X become d_x0. */
int pfc_radau_unpack_device(pfc_handle h, int n_scene, int nx, int nq, int nv, int n_ips, int n_br, const int *br_items,
                            const double *d_x0, const int *d_rule, const int *d_istate, double *d_X, double *d_q, double *d_v, double *d_s,
                            void *stream);

/* The end of an attempt, for every scene whose attempt is open and which is not iterating any more (solveRadau_inner,
 * radau_solve.jl:8-30; adaptive.jl).  params = {tol_a, tol_r, h_max, h_min} (host); mrp_off (host): the offsets in q of the n_mrp
 * floating joints' MRPs.  d_F: pfc_radau_newton_device's d_F_save, the F_k of the attempt's last iteration.  d_x, d_t, d_h, d_rule, d_cool (n_scene .. each): the committed state, time, step size, rule and cooldown,
 * updated; d_enorm (n_scene x 2): x_err_norm and x_err_norm k+1.  *d_count is set to the number of scenes armed for another attempt.
 * Attempt flag 0:
 *   update_x_err_norm!: d = (0 + (bhat0 h) xdot0) + ((bhat_k - A[NS,k]) h) F_k, k ascending (Eq. 8.17); e = factor 0 \ d (Eq. 8.19, the
 *   reference multiplies by its explicit inverse); sc_i = tol_a + max(|X_NS,i|, |x0_i|) tol_r; err = sqrt((wave sum of (e_i / sc_i)^2) / NX)
 *   (Eq. 8.21; the reference adds in index order)
 *   calc_and_update_h!: h_new = min(h_max, 2 h, ((0.9 (2 k_iter_max + 1)) / (2 k_iter_max + k_iter)) h (1 / err)^(1 / (1 + NS))), the
 *   power as sqrt or sqrt(sqrt) (the reference calls pow: rounding only); err = 0 gives 2 h; a NaN estimate is skipped by the min
 *   update_rule!: cooldown -= 1; cooldown < 1 and Psi_k < 0.1: rule = min(rule + 1, max_rule)
 *   x <- X_NS, t <- t + h, h <- h_new; principal_value! on each MRP: sigma <- -(sigma / |sigma|^2) where |sigma|^2 = (s0 s0 + s1 s1) +
 *   s2 s2 > 1 (RigidBodyDynamics' rule for SPQuatFloating, written as recalled: parity unpinned)
 * Any other attempt flag: h <- min(h_max, 2 h, 0.1 h), cooldown <- its reset value, rule <- max(rule - 1, 1); if the new h < h_min the
 * step's exit flag is 5 ("time step is too small, something is wrong": x and t stay, the scene is retired until its records are reset),
 * else the scene is armed for another attempt with the same Jacobian (its factors must be formed again: h and the rule changed).
 * PFC_ERR_BAD_ARG: the layout, the offsets, the parameters, max_rule other than 1 or 2, null buffer. */
int pfc_radau_finish_device(pfc_handle h, int n_scene, int nx, int nq, int nv, int n_ips, int n_br, const int *br_items, int n_mrp,
                            const int *mrp_off, const double *params, int k_iter_max, int max_rule, int cooldown,
                            const double *d_F, const double *d_xdot0, const double *d_X,
                            const double *d_lu0, const int *d_perm, double *d_x, double *d_t, double *d_h, int *d_rule, int *d_cool,
                            double *d_enorm, double *d_nstate, int *d_istate, int *d_count, void *stream);
/* The same with ends (what pfc_radau_step runs while an end is set, and pfc_radau_integrate always).  d_t_final (n_scene; NULL: +inf),
 * d_traj (n_scene x max_rows x (1 + NX): row r of scene s starts at (s max_rows + r) (1 + NX), t then the NX states), d_rows (n_scene:
 * the rows written so far), max_rows (0: nothing is recorded, d_traj and d_rows are not touched; 1 is PFC_ERR_BAD_ARG), d_live (one
 * word, NOT zeroed by the call).  At a commit, besides the above: the row (t, x after principal_value!) is stored at d_rows[scene] and
 * the count incremented (no row is stored where the count is not below max_rows); the scene parks -- the last word of its integer
 * record becomes 1, its step exit flag stays 0 -- if d_t_final[scene] < t or the row was the last; otherwise *d_live += 1.  Failed
 * attempts and retirements record nothing and add nothing. */
int pfc_radau_finish_end_device(pfc_handle h, int n_scene, int nx, int nq, int nv, int n_ips, int n_br, const int *br_items, int n_mrp,
                                const int *mrp_off, const double *params, int k_iter_max, int max_rule, int cooldown,
                                const double *d_F, const double *d_xdot0, const double *d_X,
                                const double *d_lu0, const int *d_perm, double *d_x, double *d_t, double *d_h, int *d_rule, int *d_cool,
                                double *d_enorm, double *d_nstate, int *d_istate, int *d_count, const double *d_t_final, double *d_traj,
                                int *d_rows, int max_rows, int *d_live, void *stream);

/*
 * The discrete controller: the reference's DiscreteControl (src/example_integrator.jl:25-30, `while ctrl.t_last <= t: ctrl.t_last +=
 * ctrl.dt; ctrl.control(x, mech_scen, t)` before every step) with a joint-space law that needs nothing but what the device holds at
 * the committed state: a computed-torque PD law with a clamp, a feed-forward torque and setpoints on a time schedule (the law of the
 * reference's test/pencil.jl, tau_ext[act] = H[act,act] qdd_des + c[act], with the schedule fixed in advance).  Zero-order hold: tau
 * changes only when the controller fires.
 * The law.  Plain Float64, no fma, in the written order; per scene, nv <= PFC_MAX_NV_SOLVE.  Coordinate i is an offset in q and in v
 * alike (they coincide for the four joint types: fixed 0 / 0, revolute 1 / 1, prismatic 1 / 1, MRP-floating 6 / 6).
 *   n_act >= 0 actuated coordinates act[0 .. n_act), strictly increasing; per actuated coordinate kp, kd and a_max (> 0; +inf: no
 *   clamp); dt, finite and > 0; per scene t_last and a schedule of n_seg >= 1 segments: seg_t (n_scene x n_seg) the start times,
 *   non-decreasing from index 1, entry 0 is not read; seg_q (n_scene x n_seg x n_act) the setpoints; seg_ff (n_scene x n_seg x nv) a
 *   feed-forward torque on every coordinate (NULL: zeros).
 *   fires = 0; while t_last <= t and fires < PFC_RADAU_MAX_FIRES: t_last = t_last + dt, fires += 1   (repeated additions, as in the
 *   reference, so the bits of t_last are the reference's).  The bound: a scene that is still due after PFC_RADAU_MAX_FIRES additions
 *   is treated as any scene that fired -- the law below, t_last as far as it got, the counter += PFC_RADAU_MAX_FIRES -- and is due
 *   again at the next call, where it goes on catching up (a dt below the spacing of t_last's neighbours never catches up: t_last +
 *   dt = t_last; the loop still ends).
 *   fires = 0: nothing of the scene is written -- tau stays byte for byte.  Otherwise, once (the law has no memory):
 *     k = the number of j in 1 .. n_seg - 1 with seg_t[j] <= t
 *     for every actuated a: e_a = q_a - seg_q[k][a];  acc_a = (-(kd_a v_a)) - kp_a e_a;  if acc_a < -a_max_a: acc_a = -a_max_a;
 *       if acc_a > a_max_a: acc_a = a_max_a   (a NaN passes)
 *     tau_a = ((..((0 + H[a,b_0] acc_b_0) + H[a,b_1] acc_b_1) ..) + c_a) + ff[k][a], b over act in increasing order
 *     tau_i = ff[k][i] for a coordinate that is not actuated
 *   H (row-major) and c are pfc_dynamics_device's outputs at (q, v).  The partials of tau stay zero: the reference's m.tau_ext is a
 *   Float64.
 * pfc_radau_control_device: the part on caller buffers and a caller stream (NULL: the handle's), asynchronous, like the other parts;
 * it reads nothing of the handle but its device and stream.  d_act (n_act ints), d_kp, d_kd, d_a_max (n_act), d_seg_t, d_seg_q,
 * d_seg_ff (or NULL) as above; d_t (n_scene), d_q (n_scene x nq), d_v (n_scene x nv), d_H (n_scene x nv x nv), d_c (n_scene x nv);
 * d_istate (n_scene x 8, pfc_radau_newton_device's records, or NULL: every scene is eligible): a scene whose step exit flag is 5 or
 * whose parked mark is set is left alone; in/out d_t_last (n_scene), d_fires (n_scene, the additions accumulate), d_tau (3 n_scene x
 * nv: the scene's rows scene, n_scene + scene and 2 n_scene + scene get the same tau).  The coordinates cannot be validated here
 * (they are device memory): the caller guarantees 0 <= act[b] < min(nq, nv), increasing.  One launch of n_scene one-wave workgroups.
 * PFC_ERR_BAD_ARG: nv outside 1 .. PFC_MAX_NV_SOLVE, nq outside 1 .. 64, n_act outside 0 .. min(nq, nv), n_seg < 1, dt not finite
 * and > 0, null buffer.
 */
#define PFC_RADAU_MAX_FIRES 4096
int pfc_radau_control_device(pfc_handle h, int n_scene, int nq, int nv, int n_act, int n_seg, double dt, const int *d_act,
                             const double *d_kp, const double *d_kd, const double *d_a_max, const double *d_seg_t, const double *d_seg_q,
                             const double *d_seg_ff, const double *d_t, const double *d_q, const double *d_v, const double *d_H,
                             const double *d_c, const int *d_istate, double *d_t_last, int *d_fires, double *d_tau, void *stream);
/*
 * pfc_radau_set_controller: the law and the schedules of the handle's batch (host arrays, sizes as above with the handle's n_scene
 * and nv; a_max NULL: +inf; seg_ff NULL: zeros; t_last0 (n_scene) NULL: every scene's current t -- the reference's constructor gives
 * 0.0 and starts at t = 0), copied into device blocks owned by the handle.  After pfc_radau_configure (PFC_ERR_STATE before it).
 * From then on every batch step of pfc_radau_step and pfc_radau_integrate begins, for the scenes that are neither retired (flag 5)
 * nor parked, with pfc_kinematics_device and pfc_dynamics_device (H and c) at the committed state and the law above; the step reads
 * tau from the device and no word is read back for it.  The attempts of one batch step share the tau of its start: the reference
 * retries inside solveRadau.  Once a controller has fired for a scene it has overwritten all nv entries of its tau, so
 * pfc_radau_set_tau only matters until the first fire (and for scenes that never fire).
 * n_act = 0 with every pointer NULL and n_seg = 0 clears the controller: the step is the step without one again -- not one launch
 * more --, with tau what pfc_radau_set_tau last set: the controller's last values if that was an array, zeros if it was NULL or never
 * called.
 * PFC_ERR_BAD_ARG, with a message and nothing changed: a coordinate out of range, not increasing, or owned by a floating or fixed
 * joint; a gain that is not finite; an a_max that is not > 0 (NaN included); dt not finite and > 0, or so small that a step of h_max
 * needs more than PFC_RADAU_MAX_FIRES additions (dt PFC_RADAU_MAX_FIRES < h_max); n_seg < 1; start times that decrease from index 1 or
 * are NaN; setpoints, feed-forward or t_last0 that are not finite.  The new blocks are allocated before the old ones are freed:
 * PFC_ERR_NOMEM leaves the previous controller in force.  pfc_radau_configure drops the controller.  pfc_radau_set_state keeps law
 * and schedule and sets every scene's t_last to its t_last0 (or its new t) and its counter to 0; a controller set before the first
 * pfc_radau_set_state takes t = 0 where t_last0 is NULL until then.
 * pfc_radau_controller_state: t_last and the additions counted per scene (n_scene each, host; either may be NULL), for tests and
 * restarts; PFC_ERR_STATE without a controller.  Multi-device handles use their first device, as the step does.
 */
int pfc_radau_set_controller(pfc_handle h, int n_act, const int *act, const double *kp, const double *kd, const double *a_max, double dt,
                             const double *t_last0, int n_seg, const double *seg_t, const double *seg_q, const double *seg_ff);
int pfc_radau_clear_controller(pfc_handle h);      /* pfc_radau_set_controller's clearing form */
int pfc_radau_controller_state(pfc_handle h, double *t_last, int *fires);

/*
 * Continuous joint feedback: the reference's continuous_controller(tm, t), called inside calcXd!
 * (src/contact_algorithms_non_friction.jl:29) at every stage evaluation with that stage's time and on the Dual state of every
 * Jacobian chunk, so that its torque is part of the differential equation and its partials are part of the matrix Radau factors.
 * The law is the discrete controller's computed-torque PD above with the same tables (act, kp, kd, a_max, seg_t, seg_q, seg_ff),
 * evaluated continuously instead of at clock ticks: no dt, no t_last.  Plain Float64, no fma, in the written order.
 * The value, per row (a scene or a stage-scene; row r reads the schedule of scene r % n_scene; nq = nv):
 *   k = the number of j in 1 .. n_seg - 1 with seg_t[j] <= t
 *   for every actuated a: acc_a = (-(kd_a v_a)) - kp_a (q_a - seg_q[k][a]);  if acc_a < -a_max_a: acc_a = -a_max_a;  if acc_a >
 *     a_max_a: acc_a = a_max_a   (a_max NULL: no clamp; a NaN passes)
 *   law_a = ((..((0 + H[a,b_0] acc_b_0) + H[a,b_1] acc_b_1) ..) + c_a) + ff[k][a], b over act in increasing order, ff = 0.0 where
 *     seg_ff is NULL: computed_torque_pd's tau_a
 *   an actuated coordinate: tau_out_a = law_a + tau_in_a, or law_a where tau_in is NULL
 *   a coordinate i that is not actuated: with seg_ff given tau_out_i = ff[k][i] + tau_in_i (ff[k][i] where tau_in is NULL); with
 *     seg_ff NULL tau_out_i is tau_in_i copied -- not added to zero, so a signed zero survives -- and +0.0 where tau_in is NULL
 * The partials, per (row, direction): the value statement instantiated on the (value, partial) number of the Dual kinematics and
 * dynamics, product rule d(a b) = da b + a db, no fma; t, the tables and tau_in are constants:
 *   dacc_a = (-(kd_a dv_a)) - kp_a dq_a;  dacc_a = 0.0 where either clamp test of the value engaged
 *   dtau_a = ((..((0 + (dH[a,b_0] acc_b_0 + H[a,b_0] dacc_b_0)) + (dH[a,b_1] acc_b_1 + H[a,b_1] dacc_b_1)) ..) + dc_a, acc clamped
 *   dtau_i = 0.0 for a coordinate that is not actuated
 * pfc_feedback_device, pfc_feedback_dual_device: the parts on caller buffers and a caller stream (NULL: the handle's),
 * asynchronous, like pfc_radau_control_device; they read nothing of the handle but its device and stream.  d_act (n_act ints; the
 * caller guarantees 0 <= act[b] < nv, increasing), d_kp, d_kd, d_a_max (n_act; d_a_max may be NULL), d_seg_t (n_scene x n_seg; may be
 * NULL with n_seg = 1), d_seg_q (n_scene x n_seg x n_act), d_seg_ff (n_scene x n_seg x nv, or NULL); d_t (n_rows), d_q, d_v, d_c (n_rows
 * x nv), d_H (n_rows x nv x nv, row-major: pfc_dynamics_device's outputs), d_tau_in (n_rows x nv, or NULL), d_tau_out (n_rows x nv).
 * The Dual part: d_dq, d_dv (n_rows x n_dir x nv: the chunk's seeds; either may be NULL: zeros), d_dH (n_rows x n_dir x nv x nv) and
 * d_dc (n_rows x n_dir x nv), pfc_dynamics_dual_device's outputs; d_dtau (n_rows x n_dir x nv).  One launch each: n_rows, or n_rows
 * n_dir, one-wave workgroups, a lane per coordinate.  PFC_ERR_BAD_ARG before any launch: nv outside 1 .. PFC_MAX_NV_SOLVE, n_act
 * outside 0 .. nv, n_seg < 1, n_scene < 1, n_rows negative or no multiple of n_scene, n_dir outside 1 .. 16, null buffer.
 */
int pfc_feedback_device(pfc_handle h, int n_rows, int n_scene, int nv, int n_act, int n_seg, const int *d_act, const double *d_kp,
                        const double *d_kd, const double *d_a_max, const double *d_seg_t, const double *d_seg_q, const double *d_seg_ff,
                        const double *d_t, const double *d_q, const double *d_v, const double *d_H, const double *d_c,
                        const double *d_tau_in, double *d_tau_out, void *stream);
int pfc_feedback_dual_device(pfc_handle h, int n_rows, int n_dir, int n_scene, int nv, int n_act, int n_seg, const int *d_act,
                             const double *d_kp, const double *d_kd, const double *d_a_max, const double *d_seg_t, const double *d_seg_q,
                             const double *d_t, const double *d_q, const double *d_v, const double *d_H, const double *d_dq,
                             const double *d_dv, const double *d_dH, const double *d_dc, double *d_dtau, void *stream);
/*
 * pfc_radau_set_feedback: the law of the handle's batch (host arrays, the sizes above with the handle's n_scene and nv), copied into
 * device blocks owned by the handle.  After pfc_radau_configure (PFC_ERR_STATE before it).  From then on, in every batch step of
 * pfc_radau_step and pfc_radau_integrate, pfc_state_derivative_device on the 3 n_scene stage-scenes evaluates the law between the
 * dynamics and the solve at the stage times, and every Jacobian chunk evaluates its partials (the first chunk its value as well) at
 * the scenes' t, as calcJacobian! does; the solve reads the summed tau and, in a chunk, dtau.  One launch more per Newton pass, two
 * per first chunk and one per later chunk, one per attempt for the stage times; nothing is read back.
 * The stage times are filled once per attempt, behind the factorisation (h and the rule change only between attempts): row
 * s n_scene + i is (c_s h_i) + t_i -- two roundings, no fma, the reference's table.c[i] * rr.step.h + t -- for s < NS(rule_i), t_i for
 * every other row.  pfc_radau_stage_times: the 3 n_scene doubles the last attempt used (host; zeros before the first step with this law;
 * PFC_ERR_STATE without a law and without body wrenches, below).  The summed tau (3 n_scene x nv), its partials (n_scene x n_chunk x nv) and the stage times live in the
 * law's own blocks: a handle without a law allocates what it allocated before.
 * tau.  The held tau keeps its meaning and its block: pfc_radau_set_tau, the discrete controller, the program and pfc_radau_get_tau
 * are what they were, and the law reads the held tau as its tau_in (NULL where none is in force).  The reference sums
 * ((f - c) + tau_cont) + tau_disc (`rhs = f - c + tm.tau_ext + m.tau_ext`); the device sums (f - c) + (tau_cont + tau_disc): the
 * two differ in the last bit.  A retired or parked scene is still evaluated (the shape is fixed) and still ignored: its x, t, h,
 * rule and norms stay byte for byte.
 * PFC_ERR_BAD_ARG, with a message and nothing changed (the previous law stays in force): a coordinate out of [0, nv), not strictly
 * increasing, or owned by a floating or fixed joint; n_seg < 1; a gain that is not finite; a negative (or NaN) a_max; start times that
 * decrease from index 1 or are NaN; setpoints or feed-forward that are not finite.  The new blocks are allocated before the old ones
 * are freed: PFC_ERR_NOMEM leaves the previous law in force.  pfc_radau_configure drops the law; pfc_radau_set_state keeps it.
 * pfc_radau_clear_feedback: the step is the step without a law again, launch for launch.  Only this law is built: arbitrary
 * callbacks stay on the host, one batch step at a time.  Multi-device handles use their first device, as the step does.
 */
int pfc_radau_set_feedback(pfc_handle h, int n_act, const int *act, const double *kp, const double *kd, const double *a_max, int n_seg,
                           const double *seg_t, const double *seg_q, const double *seg_ff);
int pfc_radau_clear_feedback(pfc_handle h);
int pfc_radau_stage_times(pfc_handle h, double *out);

/*
 * Applied body wrenches: a moment and a force on a body, acting at a point of the body's frame, on a per-scene schedule of
 * piecewise-constant segments -- a push on a box, a disturbance on a held object, a thruster that turns with its body, a random shove
 * per scene.  With the reference one writes J' w in continuous_controller; here the projection runs on the device inside the
 * differential equation, at every stage evaluation with that stage's time, and its partials -- the geometric stiffness of a
 * world-frame force at an offset point, the rotation of a body-frame follower load -- on the Dual state of every Jacobian chunk, so
 * that they are part of the matrix Radau factors.  Plain Float64, no fma, in the written order.
 * A call applies n_w wrenches.  Per wrench k, shared by all scenes: body[k] in [0, n_body); frame[k], 0: the components are along
 * the world axes, 1: along the body's axes, so that the load turns with the body; point[k], 3 doubles in the body frame.  Per scene
 * and segment: seg_w[scene][seg][k] = [moment (3); force (3)].
 * The value, per row (a scene or a stage-scene; row r reads the schedule of scene r % n_scene), with x_w_b = (R, t) (R column-major)
 * of body[k] of the row and J its Jacobian (pfc_kinematics_device's d_x_w_b and d_jac):
 *   seg = the number of j in 1 .. n_seg - 1 with seg_t[j] <= t  (the feedback law's search: a time on a start reads the new segment)
 *   [m; f] = seg_w[scene][seg][k], p = point[k]
 *   r_i = ((R_i0 p0 + R_i1 p1) + R_i2 p2) + t_i                                  the application point in world
 *   frame 1: F_i = (R_i0 f0 + R_i1 f1) + R_i2 f2, M_i likewise from m;   frame 0: F = f, M = m
 *   W = [M_i + (r x F)_i; F], (r x F)_0 = r1 F2 - r2 F1, (r x F)_1 = r2 F0 - r0 F2, (r x F)_2 = r0 F1 - r1 F0 (pfc_dynamics_device's
 *     cross product): the wrench in world about the world origin; frame 1 is transform(wrench, (R, r)) of the scatter
 *   tau_k,j = ((J0j W0 + J1j W1) + J2j W2) + ((J3j W3 + J4j W4) + J5j W5)        torque! for coordinate j
 *   tau_out_j = (..((tau_in_j + tau_0,j) + tau_1,j) ..), k ascending; where tau_in is NULL the sum starts from +0.0; n_w = 0 copies
 *     tau_in (a signed zero survives) or writes +0.0
 * The partials, per (row, direction): the same statements instantiated on the (value, partial) number of the Dual kinematics, with
 * d(a b) = da b + a db, sums componentwise, no fma; x_w_b and J are {value, dx_w_b or djac of pfc_kinematics_dual_device}; t, the
 * tables, the points and the loads are constants {x, 0.0}:
 *   dtau_out_j = (..((dtau_in_j + d tau_0,j) + d tau_1,j) ..); where dtau_in is NULL the sum starts from +0.0
 * pfc_body_wrench_device, pfc_body_wrench_dual_device: the parts on caller buffers and a caller stream (NULL: the handle's),
 * asynchronous, like pfc_feedback_device; they read nothing of the handle but its device and stream.  d_body, d_frame (n_w ints; the
 * caller guarantees 0 <= body[k] < n_body -- the kernels follow it unchecked -- and a frame other than 1 is read as 0), d_point (n_w x
 * 3), d_seg_t (n_scene x n_seg; may be NULL with n_seg = 1; entry 0 of a scene is not read), d_seg_w (n_scene x n_seg x n_w x 6), d_t
 * (n_rows), d_x_w_b (n_rows n_body x 12), d_jac (n_rows n_body x nv x 6), d_tau_in (n_rows x nv, or NULL), d_tau_out (n_rows x nv; may
 * be d_tau_in).  The Dual part: d_dx_w_b (n_rows n_body x n_dir x 12), d_djac (n_rows n_body x n_dir x nv x 6), d_dtau_in (n_rows x
 * n_dir x nv, or NULL), d_dtau (n_rows x n_dir x nv).  One launch each: n_rows, or n_rows n_dir, one-wave workgroups, a lane per
 * coordinate.  PFC_ERR_BAD_ARG before any launch: nv outside 1 .. PFC_MAX_NV_SOLVE, n_body < 1, n_w < 0, n_seg < 1, n_scene < 1,
 * n_rows negative or no multiple of n_scene, n_dir outside 1 .. 16, null buffer (with n_w = 0 the tables and the kinematics may be
 * NULL).
 */
int pfc_body_wrench_device(pfc_handle h, int n_rows, int n_scene, int n_body, int nv, int n_w, int n_seg, const int *d_body,
                           const int *d_frame, const double *d_point, const double *d_seg_t, const double *d_seg_w, const double *d_t,
                           const double *d_x_w_b, const double *d_jac, const double *d_tau_in, double *d_tau_out, void *stream);
int pfc_body_wrench_dual_device(pfc_handle h, int n_rows, int n_dir, int n_scene, int n_body, int nv, int n_w, int n_seg,
                                const int *d_body, const int *d_frame, const double *d_point, const double *d_seg_t,
                                const double *d_seg_w, const double *d_t, const double *d_x_w_b, const double *d_jac,
                                const double *d_dx_w_b, const double *d_djac, const double *d_dtau_in, double *d_dtau, void *stream);
/*
 * pfc_radau_set_body_wrenches: the wrenches of the handle's batch (host arrays, the sizes above with the handle's n_scene and the
 * mechanism's n_body), copied into device blocks owned by the handle.  After pfc_radau_configure (PFC_ERR_STATE before it).  From
 * then on, in every batch step, the chain of the 3 n_scene stage-scenes evaluates them after the dynamics and after the law, if one
 * is set, at the stage times, and every Jacobian chunk evaluates their partials (the first chunk their value as well) at the scenes'
 * t; their tau_in is the law's summed tau where a law is set and the held tau otherwise, their dtau_in the law's partials or none,
 * and the solve reads their outputs.  The right-hand side is therefore (f - c) + ((law + held) + ext_0 + ext_1 + ..), summed left to
 * right.  One launch more per Newton pass, two per first chunk, one per later chunk; the stage times (pfc_radau_set_feedback) are
 * filled once per attempt when a law or wrenches are set, and pfc_radau_stage_times answers in both cases.  The summed tau, its
 * partials and, while no law is set, the stage times live in the wrenches' own blocks: a handle without wrenches allocates what it
 * allocated before.  A retired or parked scene is still evaluated and still ignored.
 * PFC_ERR_BAD_ARG, with a message and nothing changed (the previous wrenches stay in force): n_w < 0; n_seg < 1; a body outside
 * [0, n_body); a frame other than 0 or 1; a point or a load that is not finite; start times that decrease from index 1 or are NaN.
 * The new blocks are allocated before the old ones are freed: PFC_ERR_NOMEM leaves the previous wrenches in force.
 * pfc_radau_configure drops the wrenches; pfc_radau_set_state keeps them.  pfc_radau_clear_body_wrenches: the step is the step
 * without wrenches again, launch for launch.  A wrench depends on the state through the body's pose only: springs, drag and
 * arbitrary callbacks stay on the host.  Multi-device handles use their first device, as the step does.
 */
int pfc_radau_set_body_wrenches(pfc_handle h, int n_w, const int *body, const int *frame, const double *point, int n_seg,
                                const double *seg_t, const double *seg_w);
int pfc_radau_clear_body_wrenches(pfc_handle h);

/*
 * The gripper program: the part of the reference's grip_control! that has memory (test/pencil.jl:35-116,147-173) -- a queue of
 * GripperIns instructions with durations relative to the moment each one starts, the watched body's rotation angle latched at every
 * switch, and a grip torque chosen from slip_allowed -- in front of the law above, which then runs unchanged: the program writes the
 * controller's one schedule segment, and the law's tau_a = (sum H acc + c_a) + ff_a is the reference's tau_ext[act] = H4 qdd + C4;
 * tau_ext[pad] += tau_grip.
 * The statement.  Per scene a program of n_ins >= 1 instructions and one record.  Instruction j: prog_dt[j] >= 0 (+inf allowed, never
 * NaN), prog_q[j][0 .. n_act) finite setpoints of the controller's actuated coordinates, prog_slip[j] -inf, +-0, +inf or finite (never
 * NaN).  Shared by the batch: a watched body, n_grip >= 0 grip coordinates, each one of the controller's act[], and tau_soft, tau_hard,
 * both finite.  The record: cursor = 0, pops = 0, t0 = +inf, rot_0 = +inf, angle = 0, tau_grip = 0 initially.
 * At the top of a batch step a scene runs the program if it is neither retired (exit flag 5) nor parked and t_last <= t, the
 * controller's own clock test, read before the law advances t_last.  A scene that is not due changes nothing, byte for byte.  A due
 * scene does the following once, in plain Float64, no fma, in the written order:
 *   1. R = the rotation of x_w_b[scene n_body + body] (column-major, Rij = x[(i - 1) + 3 (j - 1)]):
 *      a = R32 - R23; b = R13 - R31; c = R21 - R12;  s = sqrt((a a + b b) + c c);  w = ((R11 + R22) + R33) - 1;
 *      angle = atan2(s, w), in [0, pi]   (the reference takes AngleAxis(rotation(..)).theta of Rotations.jl 0.11.1, which is not
 *      vendored: parity unpinned, as for principal_value!)
 *   2. if t0 == +inf: t0 = t
 *   3. if cursor < n_ins - 1 and prog_dt[cursor] < (t - t0): cursor += 1, pops += 1, t0 = t, rot_0 = angle   (strict <, the
 *      reference's; one pop per step at most, also the reference's; the last instruction never expires -- a stated deviation: the
 *      reference would index an empty vector)
 *   4. sl = prog_slip[cursor]:  sl == -inf: tau_grip = 0;  sl == 0 (so -0.0 too): tau_hard;  sl == +inf: tau_soft;  otherwise
 *      tau_grip = (fabs(angle - rot_0) < sl) ? tau_soft : tau_hard   (with rot_0 = +inf, the first instruction, or a NaN angle:
 *      tau_hard, as in the reference)
 *   5. seg_q[scene][0][a] = prog_q[cursor][a] for every actuated a; seg_ff[scene][0][g] = tau_grip for every grip coordinate g (the
 *      other entries of seg_ff stay what pfc_radau_set_controller gave); then the record is stored.
 * Once per step is the reference's result: the reference calls the controller at every addition to t_last with the same (x, t), and
 * with prog_dt >= 0 a second call at the same t finds t - t0 = 0 after a pop, or an already latched t0, and changes nothing.
 * pfc_radau_program_device: the part on caller buffers and a caller stream (NULL: the handle's), asynchronous; it reads nothing of the
 * handle but its device and stream.  d_grip (n_grip ints, each < nv: the caller guarantees it), d_prog_dt and d_prog_slip (n_scene x
 * n_ins), d_prog_q (n_scene x n_ins x n_act), d_t and d_t_last (n_scene), d_x_w_b (n_scene x n_body x 12, pfc_kinematics_device's
 * output), d_istate (n_scene x 8, or NULL: every scene is eligible); in/out d_cursor (n_scene x 2: cursor, pops; the caller keeps
 * cursor in 0 .. n_ins - 1), d_pstate (n_scene x 4: t0, rot_0, angle, tau_grip), d_seg_q (n_scene x n_act) and d_seg_ff (n_scene x
 * nv).  One launch, one lane per scene.  PFC_ERR_BAD_ARG: nv outside 1 .. PFC_MAX_NV_SOLVE, n_act outside 0 .. nv, n_ins < 1, body
 * outside 0 .. n_body - 1, n_grip outside 0 .. nv, a grip torque that is not finite, null buffer.
 * pfc_radau_set_program: the program of the handle's batch (host arrays: grip (n_grip), prog_dt and prog_slip (n_scene x n_ins),
 * prog_q (n_scene x n_ins x n_act)), copied into device blocks owned by the handle; the records get their initial values.  From then on
 * the controller's part of every batch step runs the program on the handle's x_w_b after pfc_kinematics_device and before the law;
 * nothing is read back.  PFC_ERR_STATE without a controller.  PFC_ERR_BAD_ARG, with a message and nothing changed: a controller with
 * n_seg != 1 or without a seg_ff block; body outside the mechanism; a grip coordinate that is not in act[], or repeated; tau_soft,
 * tau_hard or a setpoint that is not finite; a prog_dt that is negative or NaN; a prog_slip that is NaN; n_ins < 1.  The new blocks are
 * allocated before the old ones are freed: PFC_ERR_NOMEM keeps the previous program.  pfc_radau_clear_program removes the program and
 * puts the controller's segment back to what pfc_radau_set_controller gave: the step issues the launches it issued without one.
 * pfc_radau_set_controller (any form) and pfc_radau_configure drop the program.  pfc_radau_set_state keeps the program and resets
 * every record to its initial values (and the segment to pfc_radau_set_controller's).
 * pfc_radau_program_state: the records (n_scene each, host; any pointer may be NULL); PFC_ERR_STATE without a program.  Multi-device
 * handles use their first device, as the step does.
 */
/* pfc_radau_get_tau: the tau the step reads, 3 n_scene x nv (host; the rows scene, n_scene + scene and 2 n_scene + scene of a scene are
 * equal): what pfc_radau_set_tau gave, overwritten per scene by the controller's fires; zeros where neither is in force. */
int pfc_radau_get_tau(pfc_handle h, double *tau);
int pfc_radau_program_device(pfc_handle h, int n_scene, int n_body, int nv, int n_act, int n_ins, int body, int n_grip, const int *d_grip,
                             double tau_soft, double tau_hard, const double *d_prog_dt, const double *d_prog_q, const double *d_prog_slip,
                             const double *d_t, const double *d_t_last, const double *d_x_w_b, const int *d_istate, int *d_cursor,
                             double *d_pstate, double *d_seg_q, double *d_seg_ff, void *stream);
int pfc_radau_set_program(pfc_handle h, int body, int n_grip, const int *grip, double tau_soft, double tau_hard, int n_ins,
                          const double *prog_dt, const double *prog_q, const double *prog_slip);
int pfc_radau_clear_program(pfc_handle h);
int pfc_radau_program_state(pfc_handle h, int *cursor, int *pops, double *t0, double *rot_0, double *angle, double *tau_grip);

#ifdef __cplusplus
}
#endif
#endif
