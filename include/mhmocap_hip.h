/*
 * mhmocap_hip.h -- C ABI of the MI355X-native (gfx950) scene-constrained SMPL optimisation path.
 *
 * The reference (dluvizon/scene-aware-3d-multi-human) has no FFI of its own: its boundary for
 * this path is the Python API of mhmocap/smpl.py and mhmocap/optimizer.py.  This header is the
 * thin C ABI underneath the build's Python mirror of that API
 * (scene-aware-3d-multi-human_amd/mhmocap/{smpl,optimizer,losses,...}.py binds it with ctypes;
 * INTEGRATION.md shows the binding).  Every entry point cites the reference code it replaces.
 *
 * Conventions
 *   - all functions return 0 on success, a negative mh_status otherwise; mh_last_error() gives
 *     the message of the last failure on the calling thread;
 *   - every pointer that is not marked HOST is a device pointer owned by the caller (PyTorch-ROCm
 *     allocations, tensor.data_ptr()); the library never frees or keeps caller memory and
 *     allocates nothing except the immutable model constants inside mh_model;
 *   - all floating point data is fp32 like the reference (smpl.py:134); indices are int32;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); calls only enqueue work;
 *   - a body is one (frame, person) pair; bodies are stored frame-major: b = t*N + n;
 *     a "person table" of NB rows is addressed as row (b % NB), so NB == N shares shape/scale
 *     across frames (optimizer.py:297,691) and NB == B gives per-body values (smpl.py:357).
 */
#ifndef MHMOCAP_HIP_H
#define MHMOCAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_NUM_JOINTS 24
#define MH_NUM_BETAS 10
#define MH_NUM_POSE_BASIS 207
#define MH_NUM_KP 17          /* sparse key-points of the 2D term (optimizer.py:75) */
#define MH_FEAT_STRIDE 224    /* [beta(10) | R_1..R_23 - I (207) | 0 pad] */

typedef enum mh_status {
  MH_OK = 0,
  MH_ERR_INVALID = -1,   /* bad argument */
  MH_ERR_HIP = -2,       /* a HIP runtime call failed */
  MH_ERR_NO_DEVICE = -3, /* no usable gfx950 device */
  MH_ERR_UNSUPPORTED = -4
} mh_status;

typedef struct mh_model mh_model; /* opaque: immutable SMPL constants resident in HBM */

/* HOST arrays describing an SMPL-shaped model: the fields smpl.py:201-275 reads from the pickle
 * plus the optional joint regressors of smpl.py:234-261 (NULL = absent). */
typedef struct mh_model_host {
  int32_t num_verts;            /* V (6890) */
  int32_t num_faces;            /* F (13776) */
  const float* v_template;      /* (V,3)            smpl.py:211 */
  const float* shapedirs;       /* (V,3,10)         smpl.py:227 */
  const float* posedirs;        /* (V,3,207) as in the pickle; smpl.py:264-267 reshapes it */
  const float* J_regressor;     /* (24,V) dense     smpl.py:231 */
  const float* lbs_weights;     /* (V,24)           smpl.py:274 */
  const int32_t* parents;       /* (24), parents[0] = -1   smpl.py:270-272 */
  const int32_t* faces;         /* (F,3)            smpl.py:205 */
  const float* reg_alphapose;   /* (17,V) or NULL   smpl.py:250 (already transposed)  */
  const float* reg_h36m17;      /* (17,V) or NULL   smpl.py:243 (already re-ordered)  */
  const float* reg_mupots;      /* (17,V) or NULL   smpl.py:257 */
  const float* reg_extra9;      /* (9,V)  or NULL   smpl.py:235 */
} mh_model_host;

/* joint sets of mh_joints_regress */
enum { MH_REG_ALPHAPOSE = 0, MH_REG_H36M17 = 1, MH_REG_MUPOTS = 2, MH_REG_EXTRA9 = 3 };

const char* mh_last_error(void);
int mh_version(void);

/* Measurement aid (bench.py, DESIGN.md "measurement"): when enabled, the library brackets the launches of its
 * dominant kernels with HIP events on the caller's stream; mh_profile_read synchronises on the pair of the most recent
 * launch and returns its duration.  Off by default; not meant to be on during stream capture.  on = 2 additionally
 * switches on the work counters inside the kernels (mh_raster_pair_counters); their stores cost the kernel a few percent. */
enum mh_profile_kernel {
  MH_PROF_RASTER_STRIP = 0, MH_PROF_RASTER_GRADS = 1, MH_PROF_SKIN_FWD = 2, MH_PROF_SKIN_BWD = 3,
  MH_PROF_CONTACT_KNN = 4, MH_PROF_RASTER_SUMS = 5,
  /* the rest of the "LBS + projection" unit of SURVEY 8(d) (round 4) */
  MH_PROF_POSE_FWD = 6, MH_PROF_KEYPOINTS = 7, MH_PROF_POSE_BWD = 8 /* k_pose_bwd + k_person_reduce */,
  MH_PROF_RASTER_PREP = 9 /* k_raster_prepare + k_raster_lists */, MH_PROF_COUNT = 10
};
int mh_profile_enable(int on);
int mh_profile_read(int which, float* ms);
/* number of visible HIP devices (0 on a CPU-only host; never fails) */
int mh_device_count(void);

/* Streams and the hardware queues behind them (csrc/mh_streams.hip).  The captured cycle (optimizer.py:375-602 as one
 * hipGraph) runs its chain, its side branch and the scene update of optimizer.py:578-584 on three streams; the runtime
 * multiplexes streams onto a few hardware queues, and two of the three on one queue run one after the other.
 * mh_stream_create: a NEW runtime stream (non-blocking), already bound to its queue; mh_streams_share_queue: shared = 1
 * when a and b (NULL = the default stream) drain through the same hardware queue (a spin kernel of spin_us on a, an
 * empty one on b: in-order queues show it); both synchronise.                                                        */
int mh_stream_create(void** out_stream);
int mh_stream_destroy(void* stream);
int mh_streams_share_queue(void* stream_a, void* stream_b, float spin_us, int* shared);
/* one spin kernel (one thread) of ~spin_us on the stream, asynchronous: keeps the stream's hardware queue busy */
int mh_stream_spin(void* stream, float spin_us);

/* replaces SMPL.__init__ (smpl.py:124-275): uploads and re-lays the constants once. */
int mh_model_create(mh_model** out, const mh_model_host* host);
int mh_model_destroy(mh_model* m);
/* device pointer to the (F,3) int32 face table (optimizer.py:73-74) */
const int32_t* mh_model_faces(const mh_model* m);

/* ---- a2-a6: batched LBS forward (smpl.py:490-576 + optimizer.py:702-703) -------------------
 * verts[b] = s * LBS(beta[b%NB], pose[b]) + transl[b],  s = 1.1^xscale[b%NB]
 * xscale == NULL -> s = 1; transl == NULL -> 0.
 * vposed (B,V,3) (rest-pose vertices after the blend shapes, kept for the backward) may be NULL.
 * posed_joints (B,24,3) = joints_smpl24 (smpl.py:362) without scale/translation, may be NULL.
 * ws: workspace of mh_lbs_workspace_bytes(B) bytes (keeps per-body joint transforms).       */
size_t mh_lbs_workspace_bytes(int B);
int mh_lbs_forward(const mh_model* m, int B, int NB, const float* betas /*(NB,10)*/,
                   const float* poses /*(B,72)*/, const float* xscale /*(NB) or NULL*/,
                   const float* transl /*(B,3) or NULL*/, float* verts /*(B,V,3)*/,
                   float* vposed /*(B,V,3) or NULL*/, float* posed_joints /*(B,24,3) or NULL*/,
                   void* ws, void* stream);

/* lbs(..., pose2rot=False) (smpl.py:490-491, 553-558): the 24 joint rotations are given as matrices
 * rotmats (B,24,3,3) instead of axis-angle vectors.  mh_lbs_forward_ex: either input form, and v_posed kept for
 * mh_lbs_backward_ex.                                                                                         */
int mh_lbs_forward_ex(const mh_model* m, int B, int NB, const float* betas, const float* poses /*or NULL*/,
                      const float* rotmats /*or NULL*/, const float* xscale, const float* transl, float* verts,
                      float* vposed /*or NULL*/, float* posed_joints /*or NULL*/, void* ws, void* stream);
int mh_lbs_forward_rotmats(const mh_model* m, int B, int NB, const float* betas, const float* rotmats /*(B,24,3,3)*/,
                           const float* xscale, const float* transl, float* verts, float* posed_joints /*or NULL*/,
                           void* ws, void* stream);

/* ---- the "LBS + projection" form of the forward (round 4): what the rasteriser needs of the vertices is produced in the
 * skinning epilogue, where they are in registers -- NDC projection (transforms.py:222-255 with PyTorch3D's R = diag(-1,-1,1);
 * the same three roundings per coordinate as the stand-alone projection pass of mh_raster_terms), the body's screen
 * bounding box, whether a vertex has left the pixel-row band its face lists were sorted for, and the lowest vertex
 * (arg max of y, first index on ties: optimizer.py:487-489).  mh_raster_forward_targets fills the struct for a raster
 * workspace; mh_raster_terms_projected then skips its own pass over the vertices.
 * Box and lowest vertex are found WITHOUT cross-lane reductions: a vertex only reports (one atomic min / max) when it
 * lies beyond the previous launch's extreme minus `slack`; an extreme nobody reported is left at its reset value and the
 * consumer falls back to a scan of that body (mh_raster_terms_projected / mh_lowest_resolve), so any content of the
 * previous-launch arrays gives exact results -- it only decides how many vertices report.                     */
typedef struct mh_fwd_proj {
  float s, w1, h1;             /* x_ndc = s * (-x) / z + w1, y_ndc = s * (-y) / z + h1                      */
  float ra, rk, thr;           /* pixel row = fma(-y_ndc, rk, ra); a vertex has moved when |row - rowb| >= thr */
  float slack_ndc, slack_y;    /* report when beyond (previous extreme -/+ slack): NDC units / metres        */
  float thr_soft;              /* from |row - rowb| >= thr_soft on the body's face lists are sorted again OFF the chain, beside
                                  this cycle's gradient kernel, for the next launch; from thr on: now.  thr_soft = thr: no
                                  deferred sorts                                                                 */
  float* ndc;                  /* (B,V,3) out: x_ndc, y_ndc, z                                              */
  const float* rowb;           /* (B,V)   in : pixel row of every vertex at the body's last face sort        */
  int32_t* bbox;               /* (B,4)   out: order-preserving int of min x, min y, max x, max y (z > 1e-8 only);
                                                untouched entries stay at INT_MAX / INT_MIN                  */
  int32_t* bbox_prev;          /* (B,4)   the previous launch's bbox (copied, then bbox reset, by the launch itself) */
  unsigned long long* lowkey;  /* (B)     out: order-preserving bits of y << 32 | ~vertex, 0 = nobody reported */
  unsigned long long* lowkey_prev; /* (B) */
  int32_t* moved;              /* (2B)    out: [b] = 1: some vertex left its band (thr); [B + b] = 1: some vertex is on its way
                                                out (thr_soft).  Plain stores: thousands of vertices of a body report the same */
  float* clear;                /* or NULL: clear_n floats zeroed by the launch's first kernel -- the cycle's gradient buffer,
                                  so that a captured cycle starts with the pose kernel instead of a fill + a gap        */
  unsigned long long clear_n;
} mh_fwd_proj;
int mh_lbs_forward_proj(const mh_model* m, int B, int NB, const float* betas, const float* poses,
                        const float* xscale, const float* transl, float* verts, float* vposed /*or NULL*/,
                        const mh_fwd_proj* proj, void* ws, void* stream);
/* low_idx / low_xyz of mh_lowest_vertex from the keys of mh_lbs_forward_proj (a body nobody reported for is scanned) */
int mh_lowest_resolve(const float* verts /*(B,V,3)*/, int B, int V, unsigned long long* lowkey /*(B): a missing key is written back*/,
                      int32_t* low_idx /*(B)*/, float* low_xyz /*(B,3)*/, void* stream);

/* Arithmetic of the two dense contractions of the LBS pair (pose/shape blend and its adjoint):
 * split16 = 1 (default): operands carried as two 16-bit terms, three products on the 16-bit matrix pipe with fp32
 * accumulation -- fp16 terms in the forward (vertices within ~1e-7 m of the fp32 result), bf16 terms in the backward
 * (gradients within ~2e-5 relative).  split16 = 0: exact fp32 MFMA (the round-1 kernels; A/B reference, 3-4x slower).
 * Process-wide; also selectable with MHHIP_LBS_FP32=1 in the environment before the first call.             */
int mh_lbs_set_mode(int split16);
int mh_lbs_get_mode(void);
/* mh_lbs_forward_proj as a kernel that is software-pipelined over a wave's vertex tiles (tile i's skinning / projection
 * epilogue issued between the matrix instructions of tile i + 1; on = 1, default) or tile after tile (0): the same bits
 * either way; any other value is an invalid argument.  MHHIP_FWD_PIPE=0 in the environment before the first call selects
 * 0, any other value 1.  Process-wide.                                                                                */
int mh_lbs_set_forward_pipeline(int on);
int mh_lbs_get_forward_pipeline(void);

/* sparse joint regression from vertices (smpl.py:603-620, 367-386):
 * joints[b][j] = sum_v R[j][v] * verts[b][v]  (+ (1 - rowsum_j) * corr[b] when corr != NULL,
 * which turns regression of translated/scaled vertices into s*R*x + t exactly).
 * root_relative_to >= 0 subtracts that joint (h36m17: 14, smpl.py:371-372).                 */
int mh_joints_regress(const mh_model* m, int which, int B, const float* verts /*(B,V,3)*/,
                      const float* corr /*(B,3) or NULL*/, int root_relative_to,
                      float* joints /*(B,J,3)*/, void* stream);

/* ---- the 2D key-point term without a pass over the vertices (round 4; csrc/mh_keypoints.hip) -----------------------------
 * joints_alphapose (smpl.py:374-376), scaled and translated (optimizer.py:701-703), projected (transforms.py:57-95) and
 * compared with the detections (optimizer.py:364-368, 404, 419-420) -- evaluated from what mh_lbs_forward left in `ws`
 * (pose features, joint transforms): the regressed key-points are linear in those, the constants per (key-point, bone)
 * pair are built by mh_model_create.  kp (B,17,3), uv (B,17,2) or NULL, gkp (B,17,3) = dL/dkp or NULL, loss (B).
 * ws2 != NULL: the term's adjoint (dL/d joint transforms, dL/d pose features, dL/d translation) goes into the extra
 * chunk slot of the LBS backward's workspace; mh_lbs_backward_kp then runs the skinning adjoint without key-points and
 * adds that slot.  kp_ws: mh_keypoint_workspace_bytes(m, B) bytes of scratch.                                    */
size_t mh_keypoint_workspace_bytes(const mh_model* m, int B);
int mh_keypoint_terms(const mh_model* m, int B, const float* transl /*(B,3) or NULL*/, const float* K_host,
                      const float* Kd_host /*or NULL*/, const float* joint_w_host /*[17] or NULL*/,
                      const float* pose2d /*(B,17,3)*/, float thr, float img_w, float img_h, float coef,
                      float* kp, float* uv, float* gkp, float* loss, const void* ws, void* ws2 /*or NULL*/,
                      void* kp_ws, void* stream);
int mh_lbs_backward_kp(const mh_model* m, int B, int NB, const float* betas, const float* poses,
                       const float* vposed, const float* gverts, float* gposes, float* gtransl,
                       float* gbetas, float* gxscale, void* ws, void* ws2, void* stream);
/* the same, with the rasteriser's closing job (mh_raster_fin, below; or NULL) carried out by one more workgroup of the pose
 * kernel */
typedef struct mh_raster_fin mh_raster_fin;
int mh_lbs_backward_kp_fin(const mh_model* m, int B, int NB, const float* betas, const float* poses,
                       const float* vposed, const float* gverts, float* gposes, float* gtransl,
                       float* gbetas, float* gxscale, void* ws, void* ws2, const mh_raster_fin* fin, void* stream);

/* With gbetas == gxscale == NULL the backward entries leave the shape / log-scale gradients per BODY in ws2 and skip
 * the launch that sums them over a person's frames; these two entries are the other half: where those rows are (for
 * mh_rmsprop_step_person, which sums them inside the update's launch), and the sum as a launch of its own (+= into gbetas
 * (NB,10) and gxscale (NB), NULL = skip; same order and bits as the undeferred backward).  B and the LBS arithmetic mode
 * must be those of the backward call.                                                                                  */
int mh_lbs_backward_person_partials(const mh_model* m, int B, void* ws2, float** gbeta_b, float** gxs_b);
int mh_lbs_person_reduce(const mh_model* m, int B, int NB, void* ws2, float* gbetas, float* gxscale, void* stream);

/* ---- LBS backward (hand-written adjoint of the above) ---------------------------------------
 * In : gverts (B,V,3) = dL/dverts, gjoints (B,17,3) = dL/d(alphapose joints of the translated,
 *      scaled body) or NULL, vposed from the forward, the same parameters, ws from the forward.
 * Out: gposes (B,72) [+=], gtransl (B,3) [+=], gbetas (NB,10) [+=], gxscale (NB) [+=].
 * Accumulates (+=) so that several loss terms / the priors can share one gradient buffer, like
 * autograd accumulation across the reference's per-batch backward() calls (optimizer.py:544).
 * ws2: workspace of mh_lbs_backward_workspace_bytes(B) bytes.                               */
size_t mh_lbs_backward_workspace_bytes(int B);
int mh_lbs_backward(const mh_model* m, int B, int NB, const float* betas, const float* poses,
                    const float* xscale, const float* transl, const float* vposed,
                    const float* gverts, const float* gjoints, float* gposes, float* gtransl,
                    float* gbetas, float* gxscale, void* ws, void* ws2, void* stream);
/* The same with the inputs / outputs smpl.py's autograd also covers: exactly one of `poses` (axis-angle, gposes) and
 * `rotmats` ((B,24,3,3) as given to mh_lbs_forward_rotmats -- lbs(pose2rot=False), smpl.py:541-558 -- with grotmats
 * (B,24,9) +=); gposed (B,24,3) or NULL: dL/d(posed joints) = joints_smpl24 of SMPL.forward (smpl.py:362, 735). */
int mh_lbs_backward_ex(const mh_model* m, int B, int NB, const float* betas, const float* poses, const float* rotmats,
                       const float* vposed, const float* gverts, const float* gjoints, const float* gposed,
                       float* gposes, float* grotmats, float* gtransl, float* gbetas, float* gxscale,
                       void* ws, void* ws2, void* stream);
/* adjoint of mh_joints_regress for any of the four regressors (smpl.py:367-386 under autograd; optimizer.py:41, 75, 695-696
 * with another smpl_sparse_joints_key): gverts (B,V,3) += reg^T gjoints; gcorr (B,3) += the EXPLICIT share of the
 * translation correction: sum_j (1 - rowsum_j) gjoints_j for plain joints, sum_j (1 - rowsum_j + rowsum_root) gjoints_j
 * for joints relative to a root (the rest of d/dt reaches the translation through gverts).  NULL when the joints were
 * regressed without a correction.  Deterministic (no atomics). */
int mh_joints_regress_backward(const mh_model* m, int which, int B, const float* gjoints /*(B,J,3)*/, int root_relative_to,
                               float* gverts, float* gcorr, void* stream);

/* ---- a11/a12: pinhole projection of the 17 key-points + masked 2D residual ------------------
 * (transforms.py:74-95, optimizer.py:364-368, 404-405, 414-420).
 * K: HOST 3x3 row-major intrinsics; Kd: HOST 5 distortion coefficients or NULL.
 * pose2d (B,17,3) = (x, y, confidence).  mode 0 ("fit"): residual sum((c*(uv-gt)/[W,H])^2),
 * c = conf >= thr; mode 1 ("warm-up", optimizer.py:735,754-756): mean over all B*17*2 elements
 * of (c*(uv-gt))^2 in pixels, c = conf > thr.  Writes uv (B,17,2) (may be NULL), the gradient
 * gjoints (B,17,3) scaled by `coef` (overwritten) and per-body loss partials loss (B).      */
int mh_project_joints_loss(int B, const float* joints /*(B,17,3)*/, const float* K_host,
                           const float* Kd_host, const float* pose2d, float thr, int mode,
                           float img_w, float img_h, float coef, float* uv, float* gjoints,
                           float* loss, void* stream);

/* the same with per-key-point weights joint_w (HOST, 17 floats, or NULL = all ones): the reference multiplies the
 * confidence mask by `pose17j_weights` normalised to mean 1 (optimizer.py:75-130, 259, 419-420).           */
int mh_project_joints_loss_w(int B, const float* joints, const float* K_host, const float* Kd_host,
                             const float* joint_w_host, const float* pose2d, float thr, int mode, float img_w,
                             float img_h, float coef, float* uv, float* gjoints, float* loss, void* stream);

/* a9 warm-up (optimizer.py:710-770): only poses_T is a leaf there, so the 17 key-points of every
 * body are computed ONCE (mh_lbs_forward + mh_joints_regress) and each Adam iteration is
 * joints = 1.1^xscale[b%NB] * local + transl -> projection -> mean-reduced pixel residual
 * (optimizer.py:754-756) -> gtransl (B,3) = coef * d loss / d transl (overwritten), loss (B).  */
int mh_warmup_project(int B, int NB, const float* local_joints /*(B,17,3)*/, const float* xscale,
                      const float* transl /*(B,3)*/, const float* K_host, const float* Kd_host,
                      const float* pose2d, float thr, float coef, float* gtransl, float* loss,
                      void* stream);

int mh_warmup_project_w(int B, int NB, const float* local_joints, const float* xscale, const float* transl,
                        const float* K_host, const float* Kd_host, const float* joint_w_host, const float* pose2d,
                        float thr, float coef, float* gtransl, float* loss, void* stream);

/* ---- a20: optimiser updates (optimizer.py:355-356, 586-587, 738-739, 764-765) --------------- */
int mh_rmsprop_step(float* params, const float* grads, float* square_avg, float* momentum_buf,
                    size_t n, float lr, float alpha, float momentum, float eps, void* stream);
/* mh_rmsprop_step, and in the same launch nlog floats copied from log_src to log_dst: the captured
 * cycle writes its loss sums to a staging row at a fixed address, the row of the log they belong
 * to changes every cycle (optimizer.py:588-590 appends a dict per cycle); nlog = 0: no copy.    */
int mh_rmsprop_step_log(float* params, const float* grads, float* square_avg, float* momentum_buf,
                        size_t n, float lr, float alpha, float momentum, float eps,
                        const float* log_src, float* log_dst, int nlog, void* stream);
/* mh_rmsprop_step_log, and in the same launch up to two 32-bit words written to poke_dst[0 .. npoke): the
 * device-resident switches the NEXT captured cycle reads (which of the two scene grids is live: the scene
 * is rebuilt every cycle from cycle 30 on, optimizer.py:578-584, and one captured graph serves the whole
 * fit) travel with the update instead of in a launch of their own.  npoke = 0: mh_rmsprop_step_log.     */
int mh_rmsprop_step_log_poke(float* params, const float* grads, float* square_avg, float* momentum_buf,
                             size_t n, float lr, float alpha, float momentum, float eps,
                             const float* log_src, float* log_dst, int nlog, int32_t* poke_dst, int npoke,
                             int32_t poke0, int32_t poke1, void* stream);
/* The update that also closes the LBS backward (round 6).  mh_lbs_backward* called with gbetas == gxscale == NULL
 * leaves the shape / scale gradients as per-body rows in its workspace (mh_lbs_backward_person_partials) and skips
 * the launch that sums them over the frames of a person; this entry does those sums -- same order, same bits --
 * in NB * (nbeta + 1) extra workgroups of the update's launch, adds each to its element of grads (which is
 * therefore written: not const) and updates the element.  One launch and one launch gap less at the end of every
 * optimisation cycle (optimizer.py:343-356, 586-587).  off_xscale < 0: the scale sums are dropped (the reference
 * zeroes that gradient when optim_scale_factor is off).  Everything else: mh_rmsprop_step_log_poke.             */
typedef struct mh_person_sums {
  const float* gbeta_b;   /* [>= B][nbeta] per-body shape gradients (device) */
  const float* gxs_b;     /* [>= B]        per-body log-scale gradients      */
  int B, NB, nbeta;       /* bodies (frame-major: body b belongs to person b % NB), people, shape components */
  long long off_betas;    /* element offset of the (NB, nbeta) shape leaf in params / grads */
  long long off_xscale;   /* of the (NB) scale leaf; < 0: leave it alone */
} mh_person_sums;
int mh_rmsprop_step_person(float* params, float* grads, float* square_avg, float* momentum_buf, size_t n,
                           float lr, float alpha, float momentum, float eps, const float* log_src,
                           float* log_dst, int nlog, int32_t* poke_dst, int npoke, int32_t poke0,
                           int32_t poke1, const mh_person_sums* person, void* stream);
/* the same update with the learning rate resident on the device (lr_dev[0]); afterwards
 * lr_dev[0] *= gamma (ExponentialLR).  No host scalar changes between calls, so the whole cycle can
 * be captured in a hipGraph and replayed.                                                      */
int mh_rmsprop_step_dev(float* params, const float* grads, float* square_avg, float* momentum_buf,
                        size_t n, float* lr_dev, float gamma, float alpha, float momentum, float eps,
                        void* stream);
int mh_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                 int step, float lr, float beta1, float beta2, float eps, void* stream);

/* ---- a19: one-euro filter over the leading (time) axis (optimizer.py:664-675,
 * one_euro_filter.py:32-53 with d_cutoff = 1): x (T,E) -> y (T,E), E independent channels.  */
int mh_one_euro_scan(const float* x, float* y, int T, size_t E, float min_cutoff, float beta,
                     float frame_rate, void* stream);

/* frame-sharded form: this rank holds frames [first_frame, first_frame+T) of the sequence.
 * time_before = the float32 running time stamp after frame first_frame-1 (host-computable),
 * xprev_in / dxprev_in (E) = filtered value and filtered derivative of frame first_frame-1 from
 * the previous rank (NULL on the first rank); dxprev_out (E) = state handed to the next rank
 * (its xprev is y[T-1]).                                                                      */
int mh_one_euro_scan_shard(const float* x, float* y, int T, size_t E, float min_cutoff, float beta,
                           float frame_rate, int first_frame, float time_before,
                           const float* xprev_in, const float* dxprev_in, float* dxprev_out,
                           void* stream);

/* ---- a18: temporal terms (optimizer.py:560-575) ---------------------------------------------
 * velocity: loss = sum_t ||pT[t]-pT[t-1]||^2 over t=1..T-1; gpT += coef * d loss.
 * prev_halo / next_halo (N,3): poses_T of the frame before the first / after the last local
 * frame when the sequence is sharded over GPUs (NULL at the sequence ends).  The pair
 * (t-1,t) is owned by the rank that owns frame t.  loss_out: 1 float (overwritten).         */
int mh_velocity_term(int T, int N, const float* pT /*(T,N,3)*/, const float* prev_halo,
                     const float* next_halo, float coef, float* gpT, float* loss_out, void* stream);
/* filtered-vertex smoothness: loss = sum ||(v[t]-v[t-1]) - (vf[t]-vf[t-1])||^2,
 * gverts += coef * d loss / d v.  E = N*V*3 floats per frame.  prev_* / next_* (E): the
 * neighbouring ranks' boundary frames (NULL at the sequence ends).  ws: device workspace of
 * mh_filtered_verts_workspace_bytes(T, E) bytes (per-block partial sums; one per engine).    */
size_t mh_filtered_verts_workspace_bytes(int T, size_t E);
int mh_filtered_verts_term(int T, size_t E, const float* verts, const float* verts_filt,
                           const float* prev_v, const float* prev_vf, const float* next_v,
                           const float* next_vf, float coef, float* gverts, float* loss_out,
                           void* ws, void* stream);
/* the same, but gverts = coef * d loss / d v (overwrites: the caller starts its vertex-gradient buffer with this
 * term instead of clearing it first) */
int mh_filtered_verts_term_init(int T, size_t E, const float* verts, const float* verts_filt,
                                const float* prev_v, const float* prev_vf, const float* next_v,
                                const float* next_vf, float coef, float* gverts, float* loss_out,
                                void* ws, void* stream);
/* mh_filtered_verts_term_init behind a device-resident switch: while live_dev[0] == 0 the term does not exist yet
 * (optimizer.py:383-392: the one-euro filters first run at cycle 50; :571-573 `if self.verts_filtered is not None`)
 * -- gverts is cleared, loss_out = 0 -- so that ONE captured launch sequence serves every phase of a fit.    */
int mh_filtered_verts_term_init_gated(int T, size_t E, const float* verts, const float* verts_filt,
                                      const float* prev_v, const float* prev_vf, const float* next_v,
                                      const float* next_vf, float coef, float* gverts, float* loss_out,
                                      const int32_t* live_dev, void* ws, void* stream);

/* ---- staging of the constant per-frame inputs (once per sequence; optimizer.py:396-409, 434) --
 * The N float {0,1} instance masks of a frame become ONE 32-bit word per pixel (bit n = person n,
 * N <= 32): 4 B/pixel instead of 4N, and the erosion of morphology.py:6-41 runs once instead of
 * once per batch per cycle.                                                                  */
int mh_pack_masks(const float* seg /*(T,N,H,W)*/, int T, int N, int H, int W,
                  uint32_t* bits /*(T,H,W)*/, float* area /*(T,N) pixel counts*/, void* stream);
int mh_erode_bits(const uint32_t* in, uint32_t* out /*must not alias*/, int T, int H, int W, void* stream);
/* pose2d_valid = (#joints with conf >= thr) >= 2, mask_valid = area >= min_area (optimizer.py:404-409) */
int mh_stage_gates(const float* pose2d /*(B,17,3)*/, const float* area /*(B)*/, int B, float thr,
                   float min_area, float* pose2d_valid /*(B)*/, float* mask_valid /*(B)*/, void* stream);

/* ---- a14 (mask part): occlusion ordering of the silhouette term (optimizer.py:450-477) -------
 * front[t][n] = bit set of the people closer than n (poses_T z, ties by index); apply[t][n] =
 * gate of the term (indexed by RANK like the reference, :472); D = sum_px (1-acc);
 * S = sum_px (1-acc)*seg_n over the full image.                                              */
int mh_sil_mask_stats(const uint32_t* bits, int T, int N, int H, int W, const float* pT /*(T,N,3)*/,
                      const float* pose2d_valid, const float* mask_valid, uint32_t* front /*(T,N)*/,
                      float* apply /*(T,N)*/, float* D /*(T,N)*/, float* S /*(T,N)*/, void* stream);
/* the same with the frame's pixel counts kept while the near-to-far ordering of its people is unchanged: tag (T) int32,
 * zero before the first call on these arrays (and after the masks changed); front / D / S must then persist between calls */
int mh_sil_mask_stats_cached(const uint32_t* bits, int T, int N, int H, int W, const float* pT,
                             const float* pose2d_valid, const float* mask_valid, uint32_t* front, float* apply,
                             float* D, float* S, int32_t* tag, void* stream);

/* ---- a17: priors (optimizer.py:523-532, 535-542) ---------------------------------------------
 * pose prior L1(valid*ref, valid*pose) per body -> body_loss (B), gposes +=;
 * shape prior T*L1(beta, beta_ref) (the reference adds batch_size*L1 per batch), gbetas +=;
 * scale regularisers, added once per batch (nbatches), gxscale +=.
 * loss3 = { T*L1(beta), (sum(s-1))^2, mean((s-1)^2) }.                                       */
int mh_prior_terms(int T, int N, int nbatches, const float* poses, const float* poses_ref,
                   const float* valid /*(T*N)*/, const float* betas, const float* betas_ref,
                   const float* xscale /*(N) or NULL*/, float coef_poses, float coef_scales,
                   float* gposes, float* gbetas, float* gxscale, float* body_loss /*(T*N)*/,
                   float* loss3, void* stream);
/* out[0] = scale * sum(x[0..n)) in a fixed order (loss logging, optimizer.py:546-554, 588-593) */
int mh_reduce_sum(const float* x, size_t n, float scale, float* out, void* stream);
/* two arrays of the same length in one launch (the depth / silhouette log entries of a cycle); each sum in the order
 * of mh_reduce_sum */
/* n <= 8 independent sums in one launch: xs / lens / outs are HOST arrays of device pointers and lengths */
int mh_reduce_sum_multi(int n, const float* const* xs, const size_t* lens, float* const* outs, void* stream);
int mh_reduce_sum2(const float* x0, const float* x1, size_t n, float scale, float* out0, float* out1,
                   void* stream);

/* ---- a15/a16: scene contact and foot sliding (optimizer.py:485-518) --------------------------- */
/* argmax over vertices of y (first index on ties) and that vertex                           */
int mh_lowest_vertex(const float* verts /*(B,V,3)*/, int B, int V, int32_t* low_idx /*(B)*/,
                     float* low_xyz /*(B,3)*/, void* stream);
/* dy[b] = (mean of the k nearest scene points).y - low_xyz[b].y; k <= 32 (reference: 32, by a
 * full argsort over M, optimizer.py:494-502); if M < k all M points are used.              */
int mh_contact_knn(const float* points /*(M,3)*/, int M, const float* low_xyz, int B, int k,
                   float* dy /*(B)*/, void* stream);
/* the same neighbours through a uniform grid over the scene cloud: build once per scene update
 * (mh_scene_grid_build: bbox, counting sort into cells), then every query visits cells in growing
 * shells until its k-th distance is final.  grid_ws: mh_scene_grid_bytes(M) bytes owned by the caller. */
size_t mh_scene_grid_bytes(int M);
int mh_scene_grid_build(const float* points /*(M,3)*/, int M, void* grid_ws, void* stream);
/* the same with the point count in device memory (written by mh_scene_points): grid_ws sized for M_cap, which is also
 * the M to pass to mh_contact_knn_grid */
int mh_scene_grid_build_dev(const float* points, const int* M_dev, int M_cap, void* grid_ws, void* stream);
int mh_contact_knn_grid(const void* grid_ws, int M, const float* low_xyz, int B, int k,
                        float* dy /*(B)*/, void* stream);
/* the same with the query = the lowest vertex of each body, taken from the keys mh_lbs_forward_proj reported (as
 * mh_lowest_resolve; low_idx / low_xyz are outputs) -- one launch instead of two                                  */
int mh_contact_knn_grid_key(const void* grid_ws, int M, const float* verts /*(B,V,3)*/, int V,
                            unsigned long long* lowkey /*(B)*/, int B, int k, int32_t* low_idx /*(B)*/,
                            float* low_xyz /*(B,3)*/, float* dy /*(B)*/, void* stream);
/* mh_contact_knn_grid_key over one of TWO grids of the same capacity M, chosen by device-resident words: sel_dev[0] = 0 --
 * there is no scene yet (optimizer.py:485 `if self.scene_pcd is not None`), nothing is read or written; otherwise grid_ws0
 * (sel_dev[1] = 0) or grid_ws1.  The scene update of cycle c builds the grid cycle c does not read (optimizer.py:578-584);
 * the words change between cycles, the captured launch does not.  lowkey NULL: the queries are low_xyz (input).     */
int mh_contact_knn_grid_sel(const void* grid_ws0, const void* grid_ws1, int M, const int32_t* sel_dev,
                            const float* verts /*(B,V,3)*/, int V, unsigned long long* lowkey /*(B)*/, int B, int k,
                            int32_t* low_idx /*(B)*/, float* low_xyz /*(B,3)*/, float* dy /*(B)*/, void* stream);
/* contact: sum |dy+0.02| per batch, gpT.y += coef * (-sign(dy+0.02)); foot sliding between
 * IN-BATCH consecutive frames (batch = frames per batch, optimizer.py:512-518), gverts +=
 * (atomic).  batch_contact / batch_foot: one value per batch (nbatches = ceil(T/batch)).     */
int mh_contact_foot_terms(int T, int N, int V, int batch, const float* verts, const int32_t* low_idx,
                          const float* low_xyz, const float* dy, float coef_contact, float coef_foot,
                          float* gpT, float* gverts, float* batch_contact, float* batch_foot,
                          void* stream);
/* the same with an explicit batch table: batch_frames[bt * batch + k] = frame at position k of batch bt (-1 = empty
 * position of a shorter batch); position k is paired with position k-1 of the same batch exactly like the reference does
 * with whatever its dataloader delivered -- with the shipped `shuffle: True` (configs/predict_mupots.yml:14,
 * predict.py:273-277) random frames of a random batch (optimizer.py:394, 512-518).  Every frame must appear at most
 * once in the table. */
int mh_contact_foot_terms_idx(int T, int N, int V, int batch, int nbatches, const int32_t* batch_frames /*(nbatches,batch)*/,
                              const float* verts, const int32_t* low_idx, const float* low_xyz, const float* dy,
                              float coef_contact, float coef_foot, float* gpT, float* gverts, float* batch_contact,
                              float* batch_foot, void* stream);
/* mh_contact_foot_terms[_idx] (batch_frames NULL: contiguous batches) behind the same switch as mh_contact_knn_grid_sel:
 * live_dev[0] = 0 -> both sums are 0 and no gradient is touched.                                                    */
int mh_contact_foot_terms_gated(int T, int N, int V, int batch, int nbatches, const int32_t* batch_frames,
                                const float* verts, const int32_t* low_idx, const float* low_xyz, const float* dy,
                                float coef_contact, float coef_foot, float* gpT, float* gverts, float* batch_contact,
                                float* batch_foot, const int32_t* live_dev, void* stream);
/* a21: pixel centres + depth -> camera-space points (H*W,3) (optimizer.py:605-612,
 * transforms.py:114-130).  K_host: HOST 3x3 intrinsics.                                       */
int mh_scene_unproject(const float* depth /*(H,W)*/, int H, int W, const float* K_host,
                       float* points /*(H*W,3)*/, void* stream);

/* ---- a24: scene aggregation on the device (optimizer.py:578-584; fhsog.py:180-202 aggegrate_scene_geometry_median;
 * utils.py:174-209 postprocess_depthmap, :91-135 fillin_values).  ws: mh_scene_workspace_bytes(T,H,W) bytes.
 * mh_scene_median: per-pixel masked median over the T frames of 1/target_disp (target_disp from the normalised
 *   disparity `depths` and the depth-range leaves, optimizer.py:425-426), backmask (T,H,W) bytes, non-zero = background;
 *   np.ma.median semantics (mean of the two middle values; 0 and mask 0 where no frame is valid).
 * mh_scene_postprocess: bilateral(1/clip(depth)) d=9 sigmaColor .05 sigmaSpace 25 (optional), Sobel edge mask of
 *   disparity and depth (> 3 x mean of the std-normalised sum), eroded twice, times ma_mask (may be NULL), then the
 *   fillin_ksize x fillin_ksize median fill looped until no masked pixel is left.
 * mh_scene_points: un-projection of the pixels with mask > 0.5 (row-major order) into points (<= H*W rows); the number
 *   of points is written to count_dev (device memory: no host synchronisation). */
size_t mh_scene_workspace_bytes(int T, int H, int W);
int mh_scene_median(int T, int H, int W, const float* depths /*(T,H,W)*/, const uint8_t* backmask /*(T,H,W)*/,
                    const float* zmin_lin /*(T)*/, const float* zmax_lin /*(T)*/, float* ma_depth /*(H,W)*/,
                    float* ma_mask /*(H,W) 0/1*/, void* ws, void* stream);
/* the same with pixel-major inputs (P = H*W rows of T frames: the frames of a pixel contiguous), T <= 2048: one wave
 * per pixel, no LDS.  Any (H, W) with H*W = number of pixel rows works: a pixel-sharded caller passes its slice. */
int mh_scene_median_t(int T, int H, int W, const float* depths_t /*(H*W,T)*/, const uint8_t* backmask_t /*(H*W,T)*/,
                      const float* zmin_lin, const float* zmax_lin, float* ma_depth, float* ma_mask, void* ws, void* stream);
/* scene_depth must not alias ma_depth: the filtered map is built and filled in scene_depth itself (round 6: no copy at the end) */
int mh_scene_postprocess(int H, int W, const float* ma_depth, const float* ma_mask, int use_bilateral, int fillin_ksize,
                         float* scene_depth /*(H,W)*/, void* ws, void* stream);
/* utils.py:91-135 looped until no masked pixel is left (optimizer.py:595-600 uses it with ksize 11 on the colour median):
 * values / mask (H,W) are updated in place; truncate != 0 stores floor(median) (integer-valued planes).
 * mh_scene_median_t with zmin_lin = zmax_lin = NULL takes the median of the raw (non-negative) values. */
int mh_scene_fill(int H, int W, int ksize, int truncate, float* values, float* mask, void* ws, void* stream);
int mh_scene_points(int H, int W, const float* K_host, const float* scene_depth, const float* mask, float* points,
                    int* count_dev, void* stream);

/* ---- a13/a14: differentiable z-buffer + soft silhouette fused with their residuals ------------
 * Replaces, per cycle, for all T*N bodies at once: Meshes -> MeshRasterizer(K=8, blur 1e-4) ->
 * zbuf[...,0]; MeshRenderer(K=4, blur 2e-5) + SoftSilhouetteShader (optimizer.py:211-232,
 * 427-431, 447-448); the masked mean-log-disparity residual (optimizer.py:425-442,
 * losses.py:19-30) and the occlusion-ordered silhouette residual (optimizer.py:450-477,
 * losses.py:33-40); and the backward of all of it into the vertices and the depth-range leaves.
 * PyTorch3D conventions: camera R = diag(-1,-1,1), NDC from transforms.py:222-255, pixel centres,
 * perspective_correct = False, clipped barycentrics, no culling.  cam_K_host: HOST 3x3.
 * In : verts (T*N,V,3) camera space; faces (F,3); bits / ebits (T,H,W) raw / twice-eroded
 *      instance-mask words; depths (T,H,W) normalised disparity; zmin_lin, zmax_lin (T);
 *      pose2d_valid (T*N); front, sil_apply, sil_D, sil_S from mh_sil_mask_stats.
 * Out: gverts (T*N,V,3) += coef * dL/dverts (atomic; may be NULL = losses only);
 *      gzmin, gzmax (T) += ; depth_body, sil_body (T*N) per-body loss values (un-weighted);
 *      ws: mh_raster_workspace_bytes(T,N,V,F,H,W) bytes of scratch (work list + the per-pixel
 *      K-nearest windows; sized for the worst case of every body filling the image, only the
 *      windows actually covered are touched); zbuf_out / alpha_out (T*N,H,W) or NULL: the rendered
 *      nearest-face depth (-1 = empty) and soft-silhouette images (inspection / data synthesis;
 *      the optimisation loop never materialises them).                                          */
size_t mh_raster_workspace_bytes(int T, int N, int V, int F, int H, int W);
int mh_raster_terms(int T, int N, int V, int F, int H, int W, const float* cam_K_host,
                    const float* verts, const int32_t* faces, const uint32_t* bits,
                    const uint32_t* ebits, const float* depths, const float* zmin_lin,
                    const float* zmax_lin, const float* pose2d_valid, const uint32_t* front,
                    const float* sil_apply, const float* sil_D, const float* sil_S,
                    float coef_depth, float coef_sil, float eps, float* gverts, float* gzmin,
                    float* gzmax, float* depth_body, float* sil_body, void* ws,
                    float* zbuf_out, float* alpha_out, void* stream);
/* the same call in two halves, so that a caller can order other writers of gverts between them: phases 1 = windows,
 * face sort, selection and the loss values (does not touch gverts; depth_body final, sil_body final only without
 * gradients), 2 = gradients into gverts / gzmin / gzmax and the final sil_body (same arguments, same ws), 3 = both */
int mh_raster_terms_phase(int T, int N, int V, int F, int H, int W, const float* cam_K_host,
                          const float* verts, const int32_t* faces, const uint32_t* bits,
                          const uint32_t* ebits, const float* depths, const float* zmin_lin,
                          const float* zmax_lin, const float* pose2d_valid, const uint32_t* front,
                          const float* sil_apply, const float* sil_D, const float* sil_S,
                          float coef_depth, float coef_sil, float eps, float* gverts, float* gzmin,
                          float* gzmax, float* depth_body, float* sil_body, void* ws,
                          float* zbuf_out, float* alpha_out, int phases, void* stream);
/* the same; phase 2 also writes the sums over the bodies of the depth / silhouette loss values (one float each, device
 * memory, may be NULL) -- the two entries of a cycle's log row (optimizer.py:546-554) without a reduction launch */
int mh_raster_terms_phase_log(int T, int N, int V, int F, int H, int W, const float* cam_K_host,
                          const float* verts, const int32_t* faces, const uint32_t* bits,
                          const uint32_t* ebits, const float* depths, const float* zmin_lin,
                          const float* zmax_lin, const float* pose2d_valid, const uint32_t* front,
                          const float* sil_apply, const float* sil_D, const float* sil_S,
                          float coef_depth, float coef_sil, float eps, float* gverts, float* gzmin,
                          float* gzmax, float* depth_body, float* sil_body, void* ws,
                          float* zbuf_out, float* alpha_out, int phases, float* log_depth, float* log_sil, void* stream);
/* the same after mh_lbs_forward_proj wrote into this workspace (mh_raster_forward_targets): projected != 0 -> the
 * preparation kernel reads the bounding boxes / motion flags the forward left instead of passing over `verts` (which
 * may then be NULL); a body whose box is incomplete is scanned from the projected vertices.  Same results, bit for bit.
 * phases here is a bit mask: 1 = preparation + selection, 2 = gradients, 4 = preparation only (windows, face lists, work
 * lists: a chain of small latency-bound launches), 8 = selection only -- so that a caller can start other work between the
 * two halves of phase 1. 128 (with 4 / 2, mh_raster_terms_deferred): the work lists -- a schedule: the kernels find every
 * tile and gradient unit with lists that are a launch old, or empty -- are not rebuilt between preparation and selection
 * but by the carrier of the closing job (mh_raster_fin.lists), for the next launch on the workspace. */
/* The rasterised terms' CLOSING job (per-body values from the tile sums, gradients of the depth-range leaves, the two log
 * sums: a few microseconds of latency-bound work in one workgroup) as a description that another launch can carry out:
 * nothing of the LBS backward reads what it writes, so mh_raster_terms_deferred leaves it here instead of launching
 * k_raster_finish between the gradient kernel and the backward, and mh_lbs_backward_kp_fin runs it as one more workgroup
 * of its pose kernel -- one launch and one dependent kernel less on the cycle's chain.  Plain pointers into the caller's
 * buffers and the rasteriser's workspace; valid until those are released. */
struct mh_raster_fin {
  int T, N, B, from_partials;
  float coef_depth;
  const int* body_first;
  const int* body_ns;
  const float* partial;
  const float* dinv;
  const float* sil_apply;
  const float* sil_D;
  const float* sil_S;
  float* sil_corr;
  float* depth_body;
  float* sil_body;
  const float* zmin_lin;
  const float* zmax_lin;
  float* gzmin;
  float* gzmax;
  float* log_depth;
  float* log_sil;
  /* phases & 128 of mh_raster_terms_deferred: the carrier also rebuilds the rasteriser's work lists (tile and gradient-unit
   * order: a schedule for the NEXT launch on that workspace) -- the parameter block it needs, opaque to the caller */
  int has_lists;
  unsigned long long lists[80];
};
int mh_raster_forward_targets(int T, int N, int V, int F, int H, int W, const float* cam_K_host, void* ws,
                              mh_fwd_proj* out);
int mh_raster_terms_projected(int T, int N, int V, int F, int H, int W, const float* cam_K_host,
                          const float* verts, const int32_t* faces, const uint32_t* bits,
                          const uint32_t* ebits, const float* depths, const float* zmin_lin,
                          const float* zmax_lin, const float* pose2d_valid, const uint32_t* front,
                          const float* sil_apply, const float* sil_D, const float* sil_S,
                          float coef_depth, float coef_sil, float eps, float* gverts, float* gzmin,
                          float* gzmax, float* depth_body, float* sil_body, void* ws,
                          float* zbuf_out, float* alpha_out, int phases, float* log_depth, float* log_sil,
                          int projected, void* stream);
/* phases & 2 without the closing kernel: its job goes to *fin_out (mh_raster_fin above) */
int mh_raster_terms_deferred(int T, int N, int V, int F, int H, int W, const float* cam_K_host,
                          const float* verts, const int32_t* faces, const uint32_t* bits,
                          const uint32_t* ebits, const float* depths, const float* zmin_lin,
                          const float* zmax_lin, const float* pose2d_valid, const uint32_t* front,
                          const float* sil_apply, const float* sil_D, const float* sil_S,
                          float coef_depth, float coef_sil, float eps, float* gverts, float* gzmin,
                          float* gzmax, float* depth_body, float* sil_body, void* ws,
                          float* zbuf_out, float* alpha_out, int phases, float* log_depth, float* log_sil,
                          int projected, mh_raster_fin* fin_out, void* stream);
/* Deterministic gradient scatter (default off; MHHIP_DETERMINISTIC=1 in the environment switches it on at first use).
 * The production kernel sums the per-pixel vertex gradients of the rasterised terms with fp32 atomics (LDS table,
 * then global): the summation order, hence the last bits, vary from run to run.  on != 0: one workgroup per body,
 * 64-bit fixed-point integer accumulation (exact, order-free), one writer per element -- dL/dverts and all six
 * gradient leaves are bit-identical between runs, ~4-5x slower for this kernel. */
/* Temporal coherence of the rasteriser's preparation: the per-body face lists (sorted by first pixel
 * row) are kept across launches and rebuilt for a body only when one of its vertices has moved `rows` pixel rows since the
 * body's last sort; tiles read their candidates `rows` further out and every face is decided from the current
 * coordinates, so the selection is bit-identical to a fresh sort.  Default 1 (MHHIP_RASTER_SORT_MARGIN overrides at
 * first use); 0 = sort every launch.  mh_raster_sort_counters: {bodies seen, bodies re-sorted}, cumulative over the
 * launches on this workspace (synchronises the stream); out_host NULL resets them (stream-ordered). */
/* A workspace must be initialised ONCE before its first launch (stream-ordered; again if its bytes were overwritten):
 * clears the control words (re-sort and pair counters, face-list tags, silhouette accumulator).
 * mh_raster_workspace_offsets: byte offsets of {window table (B x 4 int32), first key of every body (B x int64, in
 * window pixels), key array (5 x uint64 per window pixel)} for inspection tools. */
int mh_raster_workspace_init(int T, int N, int V, int F, int H, int W, void* ws, void* stream);
int mh_raster_workspace_offsets(int T, int N, int V, int F, int H, int W, size_t* out /*[3]*/);
/* work of the selection kernel, counted while mh_profile_enable(2) (level 2 = event brackets + in-kernel work counters): {launches, candidate (face, pixel-centre) pairs,
 * pairs evaluated after the depth cull}, cumulative (achieved pair tests per second); synchronises */
int mh_raster_pair_counters(int T, int N, int V, int F, int H, int W, void* ws, unsigned long long* out_host /*[3]*/, void* stream);
int mh_raster_set_sort_margin(int rows);
int mh_raster_get_sort_margin(void);
/* Deferred sorts (round 6): from `fraction` of the margin on, a body's lists are sorted again BESIDE the gradient kernel of the
 * launch that notices it, for the next launch -- off the chain of the cycle; only a jump of the whole margin inside one launch
 * still sorts in the preparation.  The keys do not depend on it (every face is decided from the current coordinates).
 * 0 or 1: no deferred sorts.  Default 0.6; MHHIP_RASTER_SORT_DEFER in the environment.  Process-wide.  At most 64
 * bodies per launch (the rest stay flagged for a later one, or reach the margin and sort in the preparation).       */
int mh_raster_set_sort_defer(float fraction);
float mh_raster_get_sort_defer(void);
/* test aid: all_even != 0 sends every round of the selection kernel down its even-split path (no depth cull, no pair list);
 * the selection keys must not depend on the path a round takes.  Process-wide; part of the cycle graphs' key. */
int mh_raster_set_path(int all_even);
int mh_raster_get_path(void);
int mh_raster_sort_counters(int T, int N, int V, int F, int H, int W, void* ws, unsigned long long* out_host /*[2]*/, void* stream);
/* {bodies seen, bodies re-sorted, of which beside the gradient kernel (deferred sorts)}, cumulative */
int mh_raster_sort_counters3(int T, int N, int V, int F, int H, int W, void* ws, unsigned long long* out_host /*[3]*/, void* stream);
/* Winners first (round 5): on != 0 (default; MHHIP_RASTER_WINNERS=0 switches it off) = when a body's face lists are sorted, the
 * faces that held one of the five keys of some pixel in the previous launch on this workspace go into a list of their own
 * that every tile of the selection kernel rasterises FIRST, so that the depth cull meets nearly final 4th keys for all other
 * faces.  An order only: the selection keys are the same bits with and without it, whatever the workspace held.
 * Process-wide; part of the cycle graphs' key. */
int mh_raster_set_winners(int on);
int mh_raster_get_winners(void);
int mh_raster_set_deterministic(int on);
int mh_raster_get_deterministic(void);

/* ---- the fitted scene as images: composite over the people of every frame ----------------------
 * Replaces the reference's look at a result -- matplotlib scatter plots of the projected vertices
 * (predict.py:195-243) -- with images computed where the fit ran.
 * ws: a rasteriser workspace on which a selection pass (phases & 1 of mh_raster_terms*) for exactly
 * these T,N,V,F,H,W has run: per body a screen window and, per window pixel, the nearest face
 * (z bits << 32 | face; mh_raster_workspace_offsets).  Read only.  N <= 32.
 * In : verts (T*N,V,3) camera space, the vertices of that pass; faces (F,3); images (T,H,W,3) u8 or
 *      NULL (= black); palette (N,3) DEVICE, in [0,1]; light HOST [3], unit, camera space: the
 *      direction the light TRAVELS -- shade = ambient + (1 - ambient) * max(0, -n.light), n the
 *      normal below: (0,0,1) is a head-light; (0,0,-1) shines at the camera from behind the scene
 *      and leaves every pixel at the ambient term (flat colours); ambient, alpha in [0,1].
 * Out (each may be NULL = skipped; all NULL is an error), per pixel of frame t:
 *   winner  = among the bodies n whose window holds the pixel and whose nearest-face key is not
 *             empty, the smallest (z, n): z compared as the float the key stores, the lower person
 *             index wins an exact tie;
 *   depth   (T,H,W)   the winner's z -- for an unoccluded body the same bits zbuf_out reports; -1 = empty;
 *   person, face (T,H,W) the winner's n and face index; -1 = empty;
 *   normal  (T,H,W,3) unit geometric normal (v1-v0)x(v2-v0) of the winning face from `verts`, flipped
 *             so that n_z <= 0 (towards the camera); 0 where the pixel is empty or the product is 0;
 *   overlay (T,H,W,3) u8 round(clamp((1-alpha) img + alpha c, 0, 255)), c = 255 palette[person] shade;
 *             empty pixels copy img;
 *   visible (T,N,V) u8 = 1 for the three vertices of every face that owns at least one pixel; the
 *             CALLER passes it zeroed.  Pixel-sampled visibility: it depends on the resolution (a
 *             face that falls between the pixel centres is not seen);
 *   coverage (T,N) i32 pixels every person owns (zeroed here; integer sums, exact in any order).     */
int mh_scene_composite(int T, int N, int V, int F, int H, int W,
                       const float* verts, const int32_t* faces, const void* ws,
                       const uint8_t* images, const float* palette, const float* light /*HOST [3]*/,
                       float ambient, float alpha,
                       float* depth, int32_t* person, int32_t* face, float* normal,
                       uint8_t* overlay, uint8_t* visible, int32_t* coverage, void* stream);

/* ---- the fit in numbers: per frame and per person, computed where the fit ran ---------------------
 * Replaces paging through the images above (and the reference's scatter plots, predict.py:141-257)
 * when the question is WHICH of T x N bodies went wrong.  Both calls are read-only on their inputs,
 * zero their outputs themselves and check their arguments before any HIP call.
 *
 * mh_fit_report_pixels: one pass over the pixels of T frames, N <= 32 people.
 * In : person, depth (T,H,W) as mh_scene_composite wrote them (-1 = empty); bits (T,H,W) of
 *      mh_pack_masks, read as UNSIGNED words (person 31 is bit 31), bits >= N and labels outside
 *      [0,N) are ignored; disp (T,H,W) the staged normalised disparity with min_z, max_z (T) DEVICE,
 *      the activations of the depth-range leaves -- all three NULL: no depth sums; scene_depth (H,W)
 *      f32 and scene_mask (H,W) u8 -- both NULL: no scene.
 * Out (one of the two may be NULL), for frame t and person n:
 *   counts[t][n] = { rendered:     pixels with person == n,
 *                    segmented:    pixels whose word has bit n set,
 *                    intersection: pixels with both,
 *                    behind:       pixels with person == n, scene_mask != 0 and
 *                                  depth > scene_depth + margin (ONE float add, then the compare);
 *                                  0 without a scene };
 *   dsum[t][n]   = { sum d, sum |d| } over the intersection pixels,
 *                  d = depth + depth_offset - 1 / (disp (1/min_z[t] - 1/max_z[t]) + 1/max_z[t]):
 *                  rendered against target depth in metres (optimizer.py:425; depth_offset is the
 *                  0.2 of optimizer.py:440, passed by the caller); both 0 without disp.
 * The counts are integer sums, exact in any order.  The two float sums have the same bits on every
 * launch: every d is evaluated in float32, clamped to +-1e9 (NaN counts as -1e9) and added as a
 * 64-BIT FIXED-POINT INTEGER of 2^-28 m (3.7e-9 m; sums up to 3.4e10 m) -- integer atomics in LDS
 * and one integer atomic per workgroup, person and sum in device memory, exact in any order -- and
 * the total is rounded to float32 once.  No float atomics.  The accumulators (16 T N bytes) are
 * obtained from and returned to the stream's memory pool (hipMallocAsync) inside the call; on a
 * device without a pool they are a plain allocation and the call waits for the stream before freeing.
 * The grid is sized by T H W, not by T: about 2048 workgroups whether T is 1 or 2000.
 *
 * mh_fit_report_verts: body against scene, one pass over the vertices of B bodies.  K: HOST 3x3.
 * A vertex (x,y,z) of camera space with z > 0 falls into pixel (floor(u), floor(v)),
 * u = fx x / z + cx, v = fy y / z + cy (pixel centres at +0.5: the inverse of mh_scene_unproject).
 * It is skipped when z <= 0, when the pixel is outside the image or when scene_mask is 0 there, and
 * it is INSIDE the scene when z - scene_depth[pixel] > margin (margin >= 0).
 *   pen_count[b] = number of such vertices; pen_max[b] = the largest z - scene_depth[pixel] among
 *   them, 0 if there are none (a maximum over the bit patterns of positive floats: exact in any order).
 * Unlike the `behind` count above this sees vertices hidden by another person or by the body itself.
 * One of the two outputs may be NULL.                                                              */
int mh_fit_report_pixels(int T, int N, int H, int W,
                         const int32_t* person, const float* depth, const uint32_t* bits,
                         const float* disp, const float* min_z, const float* max_z,
                         const float* scene_depth, const uint8_t* scene_mask,
                         float depth_offset, float margin,
                         int32_t* counts /*(T,N,4)*/, float* dsum /*(T,N,2)*/, void* stream);
int mh_fit_report_verts(int B, int V, int H, int W, const float* K /*HOST 3x3*/,
                        const float* verts /*(B,V,3)*/, const float* scene_depth /*(H,W)*/,
                        const uint8_t* scene_mask /*(H,W)*/, float margin,
                        int32_t* pen_count /*(B)*/, float* pen_max /*(B)*/, void* stream);

/* ---- scene penetration as a term of the fit: the backward half of mh_fit_report_verts ---------------
 * The reference has no such term (its only scene term, contact, looks at one vertex per body); it is
 * opt-in.  Every vertex is compared with the scene's depth map, BILINEARLY interpolated: on a planar
 * piece n . X = d of the scene the gradient of p (below) is s n + ((p + margin) / z) e_z with
 * s = D / (z n . ray) -- parallel to the plane's normal for a vertex ON the surface, tilted towards the
 * optical axis by (p + margin) / z <= (band + margin) / z for one behind it (a nearest-pixel lookup
 * has no slopes and could only push a body towards the camera).
 *
 * mh_scene_zmap: zmap[i] = mask[i] > 0.5 ? depth[i] : 0 -- the scene z-map (H,W): the post-processed
 *   scene depth where the scene mask (float32, as mh_scene_postprocess / mh_scene_points read it) is
 *   set, 0 where there is no scene.
 *
 * mh_scene_pen_term: verts (B,V,3) camera space, K HOST 3x3, zmap (H,W), margin >= 0, band > 0,
 *   edge > 0.  For a vertex (x,y,z) with z > 0:
 *     u = fx x / z + cx, v = fy y / z + cy (pixel centres at +0.5, as mh_scene_unproject and
 *     mh_fit_report_verts), i0 = floor(u - 0.5), j0 = floor(v - 0.5), a = u - 0.5 - i0,
 *     b = v - 0.5 - j0; taps D00 = zmap[j0][i0], D10 = zmap[j0][i0+1], D01 = zmap[j0+1][i0],
 *     D11 = zmap[j0+1][i0+1].
 *   The vertex is SKIPPED (contributes nothing) unless all four taps lie inside the image, all four
 *   are > 0 and max - min of the four is <= edge (a depth discontinuity: the bilinear slope there is
 *   meaningless and huge).  Otherwise
 *     D  = (1-b)((1-a) D00 + a D10) + b((1-a) D01 + a D11),
 *     Du = (1-b)(D10 - D00) + b(D11 - D01),   Dv = (1-a)(D01 - D00) + a(D11 - D10),
 *     p  = z - D - margin,   ACTIVE iff 0 < p < band
 *   (monocular scene depth is the front surface: a body far behind it is occluded, not inside).
 *   Value: L_b = (1/V) sum_active p^2 per body; the term is coef sum_b L_b.
 *   Out: body_loss[b] = coef L_b (may be NULL); gverts (B,V,3) (may be NULL) is ADDED to, for an active
 *   vertex with g = 2 coef p / V:
 *     d/dx = -g Du fx / z,   d/dy = -g Dv fy / z,   d/dz = g (1 + (Du fx x + Dv fy y) / z^2).
 *   One lane per vertex; every vertex is owned by one lane, so the add is a plain load, add and store
 *   (no float atomics; the caller orders the launch behind whatever else writes gverts, as with the
 *   contact term).  Everything is float32, evaluated in the order written above without fused
 *   multiply-adds.  The per-body sum of p^2 is a 64-BIT FIXED-POINT INTEGER of 2^-40 m^2 -- integer
 *   atomics in LDS, one integer atomic per workgroup and body in device memory, exact in any order --
 *   rounded to float32 once: the same bits on every launch (band^2 V < 2^23 m^2 is checked).
 *   V need not be a multiple of the workgroup (256) and a workgroup may straddle bodies.
 *   acc: accumulators owned by the caller, 8 bytes per body (8 * B bytes; cleared by the call), or NULL: obtained from
 *   and returned to the stream's memory pool inside the call, as mh_fit_report_pixels does -- not on
 *   a stream that is being captured, where NULL is an error.  Unused when body_loss is NULL.
 *
 * mh_scene_pen_term_sel: the gated form for a captured cycle, behind the same device-resident words
 *   as mh_contact_knn_grid_sel: words[0] = 0 -- no scene yet: gverts is not touched and body_loss is
 *   0; otherwise the map is zmap0 (words[1] = 0) or zmap1.                                          */
int mh_scene_zmap(int H, int W, const float* depth /*(H,W)*/, const float* mask /*(H,W) f32*/,
                  float* zmap /*(H,W)*/, void* stream);
int mh_scene_pen_term(int B, int V, int H, int W, const float* K_host /*3x3*/,
                      const float* verts /*(B,V,3)*/, const float* zmap /*(H,W)*/, float coef,
                      float margin, float band, float edge, float* gverts /*(B,V,3)*/,
                      float* body_loss /*(B)*/, void* acc /*8 * B bytes or NULL*/, void* stream);
int mh_scene_pen_term_sel(int B, int V, int H, int W, const float* K_host /*3x3*/,
                          const float* verts /*(B,V,3)*/, const float* zmap0, const float* zmap1,
                          const int32_t* words /*[scene live, which map]*/, float coef, float margin,
                          float band, float edge, float* gverts /*(B,V,3)*/, float* body_loss /*(B)*/,
                          void* acc /*8 * B bytes or NULL*/, void* stream);

/* ---- depth ordering between the people of a frame: the one term that couples two bodies -------------
 * The reference has no such term; it is opt-in.  Where the instance masks say "this pixel is person
 * y and certainly not person n", body y must be in front of body n: the depth-ordering loss of Jiang
 * et al., "Coherent Reconstruction of Multiple Humans from a Single Image" (CVPR 2020), read off the
 * nearest-face keys the rasteriser's selection pass leaves for every body SEPARATELY (slot 0 of the
 * key records, as mh_scene_composite reads them).  One streaming pass over pixels the cycle has
 * already rasterised.
 *
 * Inputs, per frame t and pixel i (row-major in H x W), for body n of the frame (b = t N + n):
 *   z_n(i) is defined exactly as k_scene_composite decides it: the body's window must lie inside the
 *     image and its keys inside the key array (T N H W records), the pixel must lie inside the window,
 *     slot 0 of the pixel's key record must not be all ones and its low word must be < F; z is the
 *     float in the high word.  A z that is not a finite positive float counts as empty.
 *   gate (T*N) float, may be NULL = every body takes part.  A body with gate[b] == 0 takes part in
 *     nothing.
 *   OWNER: person y < N with bit y of ebits[t][i] set (the twice-eroded words: confidently y), gate
 *     non-zero and z_y(i) defined.
 *   OCCLUDER of that owner: person n != y, n < N, with bit n of bits[t][i] CLEAR (the raw words:
 *     confidently not n), gate non-zero and z_n(i) defined.
 *   Words are read unsigned, so person 31 is bit 31.
 * Per (pixel, owner, occluder), all in float32, in exactly this order, with no fused multiply-add:
 *     d = (z_y - z_n) + margin;  the triple is ACTIVE iff d > 0 (the owner must be in front of everyone
 *     who is not there according to the masks, by at least margin);
 *     m = min(d, delta);  r = m * ((d + d) - m)  -- d^2 up to delta and linear beyond it, so the
 *     gradient 2 m is bounded;  r is clamped to at most 1024.
 * Sums are 64-BIT FIXED-POINT INTEGERS with q(x) = rint(x 2^24):
 *     G[y] += q(m), G[n] -= q(m);  R[y] += q(r), C[y] += 1;  if asked for, pairs[t][y][n] += 1.
 *   Integer atomics accumulate in LDS; one integer atomic per workgroup and accumulator in device
 *   memory, as mh_fit_report_pixels does it.  The sums are exact in any order: the same bits on every
 *   launch.  No float atomics anywhere.
 * Outputs, by a second launch of one lane per body:
 *     body_loss[b] = cl * float32(double(R[b]) 2^-24),  cl = float32(coef / (H W));
 *     count[b]     = C[b];
 *     gtransl[b][2] += cg * float32(double(G[b]) 2^-24), cg = float32(2 coef / (H W)) -- a plain load,
 *       add and store: the caller orders the launch against other writers of gtransl (T*N,3);
 *     pairs (T,N,N) int32 is zeroed by the call.
 *   Each output may be NULL; all NULL is an error.
 * Consequences: the gradient goes to the z of the root translation ONLY (as the contact term's goes to
 * its y only); the motion of the barycentrics with the translation, and the scale leaf, are ignored.
 * Per frame the G of all bodies sum to exactly 0.  With N == 1 nothing is active and gtransl is not
 * touched.
 * Argument checks, all before any HIP call: 0 <= margin; 0 < delta <= 1024; N <= 32; N H W <= 2^26 (a
 * body's sums then stay below 2^26 2^10 2^24 = 2^60 < 2^61 steps); T <= 65535, H <= 4095,
 * W <= 65535 (the composite's limits); no NULL table.
 *
 * mh_order_term_keys takes explicit tables as mh_raster_workspace_offsets describes them: win (T*N,4)
 *   int32 x0, y0, width, height; koff (T*N) int64 first window pixel of a body in keys; keys (T*N*H*W,5)
 *   uint64.
 * mh_order_term resolves the three offsets of a rasteriser workspace `ws` on which a selection pass
 *   for exactly these T,N,V,F,H,W has run, and calls the first.  Inside the fit's cycle the launch
 *   sits behind the selection kernel and in front of the rasteriser's gradient half: nothing runs in
 *   between on that stream, and the gradient half itself (k_raster_grads, k_raster_grads_det, the
 *   deferred face sorts that ride in it) only READS the windows and the keys -- the windows are written
 *   by k_raster_prepare and the keys by k_raster_strip alone.
 * acc: accumulators owned by the caller, 24 bytes per body (24 * T * N bytes; cleared by the call), or
 *   NULL: obtained from and returned to the stream's memory pool inside the call, as
 *   mh_scene_pen_term does -- not on a stream that is being captured, where NULL is an error.
 * Both calls own nothing and keep nothing.                                                            */
int mh_order_term_keys(int T, int N, int F, int H, int W, const int32_t* win /*(T*N,4)*/,
                       const int64_t* koff /*(T*N)*/, const uint64_t* keys /*(T*N*H*W,5)*/,
                       const uint32_t* bits /*(T,H,W)*/, const uint32_t* ebits /*(T,H,W)*/,
                       const float* gate /*(T*N) or NULL*/, float coef, float margin, float delta,
                       float* gtransl /*(T*N,3)*/, float* body_loss /*(T*N)*/, int32_t* count /*(T*N)*/,
                       int32_t* pairs /*(T,N,N)*/, void* acc /*24 * T * N bytes or NULL*/, void* stream);
int mh_order_term(int T, int N, int V, int F, int H, int W, const void* ws,
                  const uint32_t* bits /*(T,H,W)*/, const uint32_t* ebits /*(T,H,W)*/,
                  const float* gate /*(T*N) or NULL*/, float coef, float margin, float delta,
                  float* gtransl /*(T*N,3)*/, float* body_loss /*(T*N)*/, int32_t* count /*(T*N)*/,
                  int32_t* pairs /*(T,N,N)*/, void* acc /*24 * T * N bytes or NULL*/, void* stream);

/* ---- free-viewpoint render of the fit: meshes and scene point cloud, any camera ---------------------
 * The third member of the result family (mh_scene_composite: the input view as images,
 * mh_fit_report_*: the input view in numbers): the side or top view, where depth, scale and contact
 * errors show.  Replaces the reference's interactive Open3D window (mhmocap/visualization.py) on a
 * headless device.  A hard z-buffer of its own, ALL INTEGER after the projection (csrc/mh_view.hip
 * states the conventions in full); nothing of the fit's rasteriser is used.  Every call checks its
 * arguments before any HIP call, owns nothing and keeps nothing.
 *
 * Fixed point: screen in 1/64 pixel, xq = rint(u 64), yq = rint(v 64), u = fx xc / zc + cx,
 * v = fy yc / zc + cy, (xc,yc,zc) = R X + t in float32 (x right, y down, z forward); pixel (px,py) has
 * its centre at (64 px + 32, 64 py + 32).  Depth zq = rint(zc 4096), valid 1 <= zq < 2^20 (< 256 m).
 * An entry is INVALID -- written as (INT32_MIN, 0, 0) -- if zc < near (or NaN), zq is out of range or
 * |xq| or |yq| >= 2^18 (a guard band of +-4096 px).  H, W <= 4096.
 *
 * mh_view_project: count entries xyz -> out_q (xq, yq, zq) int32 under Tv <= 64 views R (Tv,3,3),
 *   t (Tv,3), K 3x3, all three HOST; near > 0.  per_view = 1: xyz holds Tv consecutive blocks of count
 *   entries, block i is projected with view i (bodies of Tv frames); per_view = 0: the same count
 *   entries under each view, out_q is (Tv,count,3) (the scene cloud).
 * mh_view_clear: keys (T,H,W) = empty (all ones).
 * mh_view_raster: draws the F faces of T N bodies, vq (T*N,V,3) from mh_view_project, into keys the
 *   caller has initialised.  A face with an invalid vertex is dropped; FACES ARE NOT CLIPPED.  Both
 *   windings are drawn, zero area is skipped.  E0, E1, E2 = integer edge functions at the pixel centre
 *   signed so that their sum A is positive: covered iff all three >= 0 (inclusive edges), depth
 *   zpix = (E0 z0 + E1 z1 + E2 z2) // A in int64 (< 2^61).  key = zpix << 32 | (n F + f), combined by
 *   ONE 64-bit unsigned atomic minimum per covered pixel: exact in any order, the same bits on every
 *   launch.  One lane per face walks a clipped box of up to 16 pixels; a larger box is drawn by the
 *   whole wave.  N <= 32, N F < 2^31.
 * mh_view_splat: draws P points pq (T,P,3) into the same keys: the square of 2 half + 1 pixels around
 *   the pixel (xq >> 6, yq >> 6), clipped to the image, at depth zq, half = min(max_half,
 *   (size_q fq // zq) // 128), size_q (P) = rint(extent in metres x 4096) (NULL or negative: 0),
 *   fq = rint(fx 64) > 0, 0 <= max_half <= 8.  key = zq << 32 | 0x80000000 | point: at an exact depth
 *   tie a mesh beats the scene, a lower person a higher one, a lower point a higher one.
 * mh_view_resolve: keys as the calls above left them -> images.  depth = zpix / 4096 (-1 = empty);
 *   label = person, -2 = scene, -1 = empty; face = face of the person / point of the scene / -1;
 *   image: 255 palette[person] shade for a person -- shade = ambient + (1 - ambient) max(0, -n.light),
 *   n the geometric normal of the face from verts_view (T*N,V,3, the vertices in VIEW space) flipped
 *   so that n_z <= 0: formula and rounding of mh_scene_composite -- point_rgb[point] (NULL: mid-grey)
 *   for the scene, background where empty; coverage[t] = pixels of person 0..N-1, then of the scene
 *   (integer sums, zeroed by the call).  palette (N,3) DEVICE; light, background HOST.  Each output
 *   may be NULL (the image's inputs may then be NULL too); all NULL is an error.                    */
int mh_view_project(int count, int per_view, int Tv, const float* xyz,
                    const float* R_host /*(Tv,3,3)*/, const float* t_host /*(Tv,3)*/,
                    const float* K_host /*3x3*/, float near, int32_t* out_q, void* stream);
int mh_view_clear(int T, int H, int W, uint64_t* keys /*(T,H,W)*/, void* stream);
int mh_view_raster(int T, int N, int V, int F, int H, int W, const int32_t* vq /*(T*N,V,3)*/,
                   const int32_t* faces /*(F,3)*/, uint64_t* keys, void* stream);
int mh_view_splat(int T, int P, int H, int W, const int32_t* pq /*(T,P,3)*/,
                  const int32_t* size_q /*(P)*/, int fq, int max_half, uint64_t* keys, void* stream);
int mh_view_resolve(int T, int N, int V, int F, int H, int W, const uint64_t* keys,
                    const float* verts_view, const int32_t* faces, const uint8_t* point_rgb /*(P,3)*/,
                    const float* palette /*(N,3) DEVICE*/, const float* light_host /*3*/, float ambient,
                    const uint8_t* background_host /*3*/, uint8_t* image /*(T,H,W,3)*/,
                    float* depth /*(T,H,W)*/, int32_t* label, int32_t* face,
                    int32_t* coverage /*(T,N+1)*/, void* stream);

/* ---- body-to-scene contact map: the nearest scene point of every vertex ----------------------------
 * The fourth member of the result family: which part of a body touches the scene and how far the
 * rest is from it -- in 3D, against the whole cloud (the contact term and contact_dy_m look at one
 * vertex per body, the penetration term along camera rays at the front surface).  The reference
 * answers this through an interactive viewer only.  Read-only, off the cycle; no term of the fit.
 *
 * mh_scene_nearest: grid_ws and M exactly as mh_contact_knn_grid takes them (a workspace
 *   mh_scene_grid_build or mh_scene_grid_build_dev has filled, M = the size it was carved for; the
 *   number of points is the count the build left on the device, so rows behind a device-side count
 *   are not part of the cloud); queries (Q,3) on the device; radius in metres.
 *   For query q and cloud point p, all in float32, in exactly this order, with no fused multiply-add:
 *       dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;   d2 = (dx dx + dy dy) + dz dz;
 *       r2 = radius radius;   p is a CANDIDATE iff d2 <= r2.
 *   d2[q] = the smallest d2 over the candidates; near_xyz[q] = the candidate that attains it, on equal
 *   d2 the one with the smallest x, then y, then z (coordinates compare as numbers: candidates that
 *   differ only in the sign of a zero are the same point).  The result is a function of the candidate
 *   SET and does not depend on the order the cloud is visited in.  Without a candidate, for a query
 *   with a coordinate that is not finite, and for an empty cloud: d2 = +inf, near_xyz = (0,0,0).
 *   Either output may be NULL, not both.
 *   One lane per query, workgroups of 256; a lane walks the rows of cells its box [q - r, q + r] can
 *   touch -- a superset of every candidate's cell under float32 rounding (csrc/mh_contact.hip argues
 *   it) -- and a query whose box misses the cloud's bounding box ends after reading the grid's header.
 *   Refused before any HIP call: Q <= 0, M <= 0, a NULL grid or queries, both outputs NULL, a radius
 *   that is not finite and positive, and a radius above MH_SCENE_NEAREST_MAX_CELLS cells of the
 *   smallest cell size a grid can have (0.02 m): 0.64 m.  A box then spans at most
 *   2 * 32 + 2 = 66 cells per axis, 66^2 rows of cells per query.
 *
 * mh_contact_parts: d2 (B,V) as mh_scene_nearest wrote it for B bodies of V vertices; part (V) uint8:
 *   the part of every vertex, the same for all bodies; P <= 32 parts; thr in metres, finite, >= 0.
 *       counts[b][k] = number of vertices v with part[v] = k and d2[b][v] <= thr thr (float32 product);
 *       min_d2[b][k] = the smallest d2[b][v] over part[v] = k, +inf for a part without a vertex (or
 *                      with none in reach).
 *   A vertex with part[v] >= P counts nowhere; a d2 that is NaN or negative is never a minimum.
 *   Integer atomics only: a count, and a minimum on the BIT PATTERN (floats >= 0 order like unsigned
 *   integers), accumulated in LDS per workgroup, then one atomic per workgroup and accumulator in
 *   device memory, as mh_fit_report_pixels does it: the same bits on every launch.  Both outputs are
 *   overwritten by the call; either may be NULL, not both.
 * Both calls own nothing and keep nothing.                                                          */
#define MH_SCENE_NEAREST_MAX_CELLS 32
int mh_scene_nearest(const void* grid_ws, int M, const float* queries /*(Q,3)*/, int Q, float radius,
                     float* d2 /*(Q)*/, float* near_xyz /*(Q,3)*/, void* stream);
int mh_contact_parts(int B, int V, const float* d2 /*(B,V)*/, const uint8_t* part /*(V)*/, int P,
                     float thr, int32_t* counts /*(B,P)*/, float* min_d2 /*(B,P)*/, void* stream);

/* ---- person-to-person contact map: the nearest OTHER body of every vertex ---------------------------
 * The one 3D result between people: do two people touch, where, with which body parts, and on which
 * side of the other's surface a vertex lies (the depth-ordering term and its report work in image
 * space, per pixel; the reference answers this through its interactive viewer only).  Read-only, off
 * the cycle; no term of the fit.  All arithmetic below is float32, every operation rounded on its
 * own, in exactly the order written, with no fused multiply-add: a float32 evaluation of the same
 * expressions on the host gives the same bits.  No float atomics anywhere: the same bits on every
 * launch.
 *
 * mh_vertex_normals: area-weighted, NOT normalised vertex normals of B bodies with the same F faces.
 *   adj_start (V+1), adj_face (A): for vertex v the faces adj_face[adj_start[v] .. adj_start[v+1]-1]
 *   that name it (mhhip.proximity.vertex_faces builds the table: ascending face index, a face once
 *   per corner that names the vertex).
 *       normals[b][v] = sum over k = adj_start[v] .. adj_start[v+1]-1, IN THAT ORDER, starting from
 *                       +0, of n(f), f = adj_face[k];
 *       with (v0, v1, v2) the vertices of face f, e1 = v1 - v0, e2 = v2 - v0:
 *       n(f) = (e1.y e2.z - e1.z e2.y,  e1.z e2.x - e1.x e2.z,  e1.x e2.y - e1.y e2.x).
 *   Only the direction is used, and leaving out the square root and the division keeps the bits
 *   reproducible.  A gather, one lane per (body, vertex).  A face index outside [0, F), or a face
 *   that names a vertex outside [0, V), contributes nothing (the range k is clipped to [0, A]); a
 *   vertex without faces gets (0, 0, 0).
 *   Refused before any HIP call: B, V or F <= 0, A < 0, B * V beyond one launch, a NULL pointer
 *   (adj_face may be NULL when A = 0).
 *
 * mh_person_nearest: verts (T,N,V,3) on the device: N bodies of V vertices in each of T frames;
 *   live (T,N) uint8 or NULL; radius in metres; ws: a workspace of at least
 *   mh_person_nearest_bytes(T, N, V) bytes, whose content before and after the call means nothing.
 *   A person n of frame t is LIVE iff live is NULL or live[t][n] != 0.
 *   For query q = verts[t][n][v] of a live person with three finite coordinates, the candidates are
 *   the p = verts[t][m][u] with m != n in the SAME frame, m live and p of three finite coordinates,
 *       dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;   d2 = (dx dx + dy dy) + dz dz;
 *       r2 = radius radius;   d2 <= r2   (a NaN d2 is no candidate).
 *   d2[t][n][v] = the smallest candidate d2; idx[t][n][v] = m V + u of the candidate that attains
 *   it, on equal d2 the smallest m, then the smallest u.  Without a candidate, for a dead person and
 *   for a query that is not finite: d2 = +inf, idx = -1.  The result is a function of the candidate
 *   SET, not of any visiting order.  Either output may be NULL, not both.
 *   One uniform grid per BODY (at most 4096 cells, cell >= 0.02 m), all built by four launches over
 *   the call (boxes, counts, scan, scatter; integer atomics only); vertices that are not finite are
 *   neither binned nor do they widen a box; a body of zero extent is one cell.  The query is one
 *   lane per vertex that walks the other bodies of its frame and drops a body whose bounding box,
 *   grown by the radius, misses it after reading that body's header; in the others it walks the
 *   rows of cells its box [q - r, q + r] can touch, a superset of every candidate's cell under
 *   float32 rounding (csrc/mh_proximity.hip argues it).
 *   Refused before any HIP call: T, N or V <= 0; N > 32; N V >= 2^31; T N V beyond what one launch
 *   can index; NULL verts or ws; ws_bytes below mh_person_nearest_bytes; both outputs NULL; a radius
 *   that is not finite and positive, or above 0.64 m (the cap of mh_scene_nearest).
 *
 * mh_person_pairs: d2, idx (T,N,V) as mh_person_nearest wrote them for verts; normals (T,N,V,3) as
 *   mh_vertex_normals wrote them for verts, or NULL; part (V) uint8, the part of every vertex, the
 *   same for all bodies; P <= 32 parts; thr in metres, finite, >= 0.
 *   For vertex v of person n with idx = m V + u >= 0, q = verts[t][n][v], p = verts[t][m][u]:
 *       IN CONTACT iff d2 <= thr thr (float32 product);
 *       BEHIND iff normals is given and, with w = normals[t][m][u],
 *           ((q.x - p.x) w.x + (q.y - p.y) w.y) + (q.z - p.z) w.z < 0.
 *   BEHIND says that the vertex lies on the inner side of the other body's surface AT THAT BODY'S
 *   NEAREST VERTEX: a cheap, local stand-in for "inside", exact in its definition.  It is NOT a
 *   winding-number (points-inside-mesh) test and can differ from one near concave regions
 *   (mh_person_inside below is that test).
 *       behind[t][n][v]      = 1 iff the vertex is behind, in contact or not; 0 where idx < 0;
 *       pair_verts[t][n][m]  = vertices of n in contact whose nearest person is m;
 *       pair_behind[t][n][m] = vertices of n in contact and behind whose nearest person is m;
 *       pair_min_d2[t][n][m] = the smallest d2 over the vertices of n whose nearest person is m,
 *                              +inf when there is none (the diagonal is 0 / +inf);
 *       part_verts[t][n][k]  = vertices in contact with part[v] = k;
 *       part_min_key[t][n][k] = the 64-bit minimum over part[v] = k, idx >= 0 of
 *                              (bits of d2 << 32 | idx), all ones when there is none: one integer
 *                              gives the part's smallest distance and the vertex of the other body it
 *                              is closest to (on equal d2 the smallest idx).
 *   A part[v] >= P counts nowhere; an idx at or beyond N V is treated as idx < 0; a d2 that is NaN
 *   or negative is never a minimum.  Integer atomics only -- counts, and minima on the BIT PATTERN
 *   (floats >= 0 order like unsigned integers) -- accumulated in LDS per workgroup, then one atomic
 *   per workgroup and accumulator in device memory, as mh_contact_parts does it.  V need not be a
 *   multiple of the workgroup.  Every output is overwritten by the call; each may be NULL, not all.
 *   Refused before any HIP call: T, N or V <= 0; N > 32; P outside 1..32; N V >= 2^31; T N V beyond
 *   one launch; NULL verts, d2, idx or part; every output NULL; thr not finite or negative.
 * The calls own nothing and keep nothing.                                                           */
int mh_vertex_normals(int B, int V, int F, const float* verts /*(B,V,3)*/, const int32_t* faces /*(F,3)*/,
                      const int32_t* adj_start /*(V+1)*/, const int32_t* adj_face /*(A)*/, int A,
                      float* normals /*(B,V,3)*/, void* stream);
size_t mh_person_nearest_bytes(int T, int N, int V);
int mh_person_nearest(int T, int N, int V, const float* verts /*(T,N,V,3)*/, const uint8_t* live /*(T,N)*/,
                      float radius, void* ws, size_t ws_bytes, float* d2 /*(T,N,V)*/,
                      int32_t* idx /*(T,N,V)*/, void* stream);
int mh_person_pairs(int T, int N, int V, const float* verts, const float* normals /*(T,N,V,3)*/,
                    const float* d2, const int32_t* idx, const uint8_t* part /*(V)*/, int P, float thr,
                    uint8_t* behind /*(T,N,V)*/, int32_t* pair_verts /*(T,N,N)*/,
                    float* pair_min_d2 /*(T,N,N)*/, int32_t* pair_behind /*(T,N,N)*/,
                    int32_t* part_verts /*(T,N,P)*/, uint64_t* part_min_key /*(T,N,P)*/, void* stream);

/* ---- points inside a mesh, and the person-to-person penetration map ---------------------------------
 * Is a point INSIDE a closed triangle mesh, and how far is the surface above and below it along z
 * (the camera axis): the winding-number test that BEHIND above is not.  Read-only, off the cycle; no
 * term of the fit.  The test is defined in integers, so it is exact, the same on every launch, and an
 * int64 evaluation of the same rules on the host gives the same bits (tests/inside_ref.py).
 *
 * LATTICE.  A coordinate x becomes X = (int32) rintf(x * 65536.0f): the scaling is exact, the rounding
 *   is half to even, the step is 2^-16 m.  All later arithmetic is integer.
 * TESTABLE BODY.  A vertex is finite iff its three coordinates are.  A body is testable iff it is
 *   live, has at least one finite vertex, every finite coordinate of every vertex satisfies
 *   |x| < 8192 m, and its lattice box over the finite vertices is at most 2^19 units (8 m) on every
 *   axis.  Any other body contains nothing; its status word says why.
 * SKIPPED FACES.  A face that names a vertex outside [0, V), or a vertex that is not finite,
 *   contributes nothing.
 * EDGE SIGN.  For the directed edge P0 -> P1 and the query Q, in int64,
 *       E = (X1 - X0) (Qy - Y0) - (Y1 - Y0) (Qx - X0);
 *       sgn = sign(E) if E != 0; else -sign(Y1 - Y0) if Y1 != Y0; else sign(X1 - X0) (0 if X1 = X0).
 *   This is the symbolic perturbation Q + (eps, eps^2): E(Q + (eps, eps^2)) = E - eps (Y1 - Y0) +
 *   eps^2 (X1 - X0).  It is antisymmetric under edge reversal, so a ray through a shared edge or a
 *   vertex is counted for exactly one of the faces around it.
 * FACE AND QUERY.  For the face (P0, P1, P2): w0 = E(P1 -> P2), w1 = E(P2 -> P0), w2 = E(P0 -> P1),
 *   A = w0 + w1 + w2 (twice the signed area of the face's projection, whatever Q is).
 *       The face COVERS Q iff A != 0 and the three edge signs are equal and not zero.
 *       Nn = w0 (Z0 - Qz) + w1 (Z1 - Qz) + w2 (Z2 - Qz)     (Nn / A = the face's z over Q, minus Qz)
 *       ABOVE iff Nn != 0 and sign(Nn) = sign(A); BELOW iff Nn != 0 and sign(Nn) != sign(A); Nn = 0
 *       (the query is on the face) is neither.  dz = |Nn| / |A|, truncated, in lattice units.
 *   Bounds: a query that is tested lies in the body's closed box, so every coordinate difference is
 *   at most 2^19 in magnitude and kept in int32; |E| <= 2 * 2^38 = 2^39; |A| <= 2^38 (twice an area
 *   inside a 2^19 square); |Nn| <= 3 * 2^39 * 2^19 < 2^61; on a covering face the w have one sign,
 *   so |Nn| <= |A| 2^19 and dz <= 2^19.
 * RESULTS per (query, body).
 *       winding = the sum over covering faces ABOVE of sign(A): +1 inside an outward-oriented closed
 *                 mesh (counter-clockwise seen from outside in a right-handed frame), -1 inside an
 *                 inward-oriented one, 0 outside either;
 *       up      = the smallest dz over covering faces ABOVE, down = over those BELOW; -1 without one.
 *   A query that is not finite, or lies outside the body's closed lattice box (a query with a
 *   coordinate at or beyond 8192 m is outside every box), has winding 0 and up = down = -1.
 *   INSIDE iff winding != 0; exit(q, m) = the smaller of up and down that exist.  Every result is a
 *   function of the face SET, never of a visiting order or of the search structure.
 *
 * mh_mesh_bins: B bodies verts (B,V,3) with the same faces (F,3); live (B) uint8 or NULL (all live).
 *   Fills ws (at least mh_mesh_bins_bytes(B, F) bytes) for mh_mesh_winding and mh_person_inside: per
 *   body the status, the lattice box, the three lattice corners of every face, and a 2D grid over
 *   the box's x and y.  The cell edge is the smallest power of two (a cell index is a shift) at which
 *   the grid has at most 64 cells per axis and at most max(F / 4, 256) cells in all; a face is listed
 *   in every cell its closed xy box overlaps (count, scan, fill; integer atomics only), so a query
 *   looks at the one cell it falls in.  The lists of a body hold at most 8 F entries; a body that
 *   needs more is marked and its queries walk all F faces -- coarse meshes of a dozen huge faces are
 *   the ones that take that path.  The results are the same either way.
 *   status[b] (may be NULL): bit 1 = not live, 2 = live but not testable (the range rules above),
 *   4 = testable and walking all faces.  A body contains nothing iff status & 3.
 *   mh_mesh_set_all_faces(1) sends every testable body of later mh_mesh_bins calls down the
 *   all-faces path (a yardstick for what the grid buys, and a test of the claim above); it returns
 *   the previous setting, and 0 restores the default.
 *   Refused before any HIP call: B, V or F <= 0; B V or 8 B F beyond one launch; NULL verts, faces or
 *   ws; ws_bytes below mh_mesh_bins_bytes.
 * mh_mesh_winding: the generic query, points (B,Q,3): point j of row b against body b of the ws that
 *   mh_mesh_bins filled for the same B, V, F and faces.  One lane per point.  winding, up, down (B,Q)
 *   int32; each may be NULL, not all.
 *   Refused before any HIP call: B, V, F or Q <= 0; B Q or 8 B F beyond one launch; NULL faces, ws or
 *   points; every output NULL.
 * mh_person_inside: verts (T,N,V,3), and ws as mh_mesh_bins filled it for THE SAME verts taken as
 *   B = T N bodies; part (V) uint8, the part of every vertex; P <= 32 parts.  One lane per vertex,
 *   which walks the other testable bodies m != n of its frame and drops a body whose box misses it
 *   after reading that body's header.
 *       mask[t][n][v]  uint32: bit m is set iff the vertex is INSIDE body m (N <= 32: one word);
 *       depth[t][n][v] = the largest exit(q, m) over the bodies in the mask, in lattice units;
 *       other[t][n][v] = the m that attains it, the smallest m on a tie; both -1 when the mask is 0;
 *       pair_verts[t][n][m] = vertices of n inside m; pair_depth[t][n][m] = the largest exit over
 *                        them, -1 if none (the diagonal is 0 / -1);
 *       part_verts[t][n][k] = vertices with part[v] = k inside anybody; part_depth[t][n][k] = their
 *                        largest depth, -1 if none.
 *   The vertices of a person that is not live get 0 / -1 / -1 and count nowhere; a part[v] >= P counts
 *   in no part.  Counts and maxima are accumulated in LDS per workgroup, then one integer atomic per
 *   workgroup and accumulator, as mh_person_pairs does it; V need not be a multiple of the
 *   workgroup.  Every output is overwritten by the call; each may be NULL, not all.
 *   Refused before any HIP call: T, N, V or F <= 0; N > 32; P outside 1..32; T N V or 8 T N F beyond
 *   one launch; NULL faces, ws, verts or part; every output NULL.
 * The calls own nothing and keep nothing beyond the switch of mh_mesh_set_all_faces.                  */
size_t mh_mesh_bins_bytes(int B, int F);
int mh_mesh_bins(int B, int V, int F, const float* verts /*(B,V,3)*/, const int32_t* faces /*(F,3)*/,
                 const uint8_t* live /*(B)*/, void* ws, size_t ws_bytes, int32_t* status /*(B)*/,
                 void* stream);
int mh_mesh_set_all_faces(int on);
int mh_mesh_winding(int B, int V, int F, const int32_t* faces, const void* ws, int Q,
                    const float* points /*(B,Q,3)*/, int32_t* winding /*(B,Q)*/, int32_t* up /*(B,Q)*/,
                    int32_t* down /*(B,Q)*/, void* stream);
int mh_person_inside(int T, int N, int V, int F, const int32_t* faces, const void* ws,
                     const float* verts /*(T,N,V,3)*/, const uint8_t* part /*(V)*/, int P,
                     uint32_t* mask /*(T,N,V)*/, int32_t* depth /*(T,N,V)*/, int32_t* other /*(T,N,V)*/,
                     int32_t* pair_verts /*(T,N,N)*/, int32_t* pair_depth /*(T,N,N)*/,
                     int32_t* part_verts /*(T,N,P)*/, int32_t* part_depth /*(T,N,P)*/, void* stream);

/* ---- exact point-to-surface distance, and the person-to-person clearance map -------------------------
 * How far is a point from the SURFACE of a triangle mesh, and which point of it is the nearest: for a
 * vertex that mh_person_inside found inside another body the shortest way out, for every other vertex
 * the clearance.  (mh_person_nearest measures to the nearest VERTEX, mh_person_inside's depth along z
 * only.)  Read-only, off the cycle; no term of the fit.
 *
 * THE DEFINITION.  Everything is float32, evaluated in the order written, without contraction, so a
 * float32 evaluation of the same expressions on the host gives the same bits (tests/surface_ref.py).
 * With dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z, the squared distance D2 from the query q to the face
 * (a, b, c) is the region method in its query-centred form:
 *     A = a - q; B = b - q; C = c - q; ab = b - a; ac = c - a
 *     d1 = -dot(ab, A); d2 = -dot(ac, A); d3 = -dot(ab, B); d4 = -dot(ac, B); d5 = -dot(ab, C);
 *     d6 = -dot(ac, C)
 *     vc = d1 d4 - d3 d2; vb = d5 d2 - d1 d6; va = d3 d6 - d5 d4; e1 = d4 - d3; e2 = d5 - d6
 *     the first region that holds, in this order, gives (v, w):
 *       d1 <= 0 && d2 <= 0               -> (0, 0)                          vertex a
 *       d3 >= 0 && d4 <= d3              -> (1, 0)                          vertex b
 *       vc <= 0 && d1 >= 0 && d3 <= 0    -> (d1 / (d1 - d3), 0)             edge ab
 *       d6 >= 0 && d5 <= d6              -> (0, 1)                          vertex c
 *       vb <= 0 && d2 >= 0 && d6 <= 0    -> (0, d2 / (d2 - d6))             edge ac
 *       va <= 0 && e1 >= 0 && e2 >= 0    -> (1 - t, t), t = e1 / (e1 + e2)  edge bc
 *       otherwise                        -> (vb / den, vc / den), den = (va + vb) + vc
 *     x = (A + ab v) + ac w  (per component);  D2 = dot(x, x);
 *     closest point = q + x;  weights = ((1 - v) - w, v, w).
 *   The differences to the query are taken first, so near the surface they are exact and the result
 *   does not lose digits with the distance from the origin.  Collinear and single-point faces give the
 *   right distance through the edge and vertex regions.
 * CANDIDATES of a query against a body: a face that names three vertices in [0, V) whose nine
 *   coordinates are finite, whose D2 is not NaN, and D2 <= r2, r2 = radius radius (float32); a radius
 *   of +inf admits every D2 that is not NaN.
 * RESULT: the smallest candidate D2; on equal D2 the smallest face index (a query on a shared edge ties
 *   between the two faces).  A function of the candidate SET, never of a visiting order or of the
 *   search structure.  A query that is not finite, a dead body, and a query without a candidate give
 *   D2 = +inf, face = -1 (and a point and weights of zeros).
 *
 * mh_surface_grid: B bodies verts (B,V,3) with the same faces (F,3); live (B) uint8 or NULL (all live).
 *   Fills ws (at least mh_surface_grid_bytes(B, F) bytes) for mh_mesh_closest and mh_person_surface:
 *   per body the box of its finite vertices, the three corners of every face (48 bytes, so a face visit
 *   is three 16-byte loads), and a 3D uniform grid of face lists over the box: cubic cells, at most 64
 *   per axis and at most min(max(F / 2, 256), 8192) in all, the smallest edge of the sequence
 *   (longest extent) / 64 * 1.0625^i that satisfies both; a face is listed in every cell its bounding box
 *   overlaps (count, scan, fill; integer atomics only).  The lists of a body hold at most 16 F entries;
 *   a body that needs more -- a coarse mesh of a dozen huge faces -- or whose box overflows float32 is
 *   marked and its queries walk all F faces.  The results are the same either way.
 *   status[b] (may be NULL): bit 1 = not live, 4 = live and walking all faces.
 *   mh_surface_set_all_faces(1) sends every live body of later mh_surface_grid calls down the
 *   all-faces path (a yardstick for what the grid buys, and a test of the claim above); it returns the
 *   previous setting, and 0 restores the default.
 *   Refused before any HIP call: B, V or F <= 0; B V or 16 B F beyond one launch; NULL verts, faces or
 *   ws; ws_bytes below mh_surface_grid_bytes.
 * mh_mesh_closest: the generic query, points (B,Q,3): point j of row b against body b of the ws that
 *   mh_surface_grid filled for the same B, V, F and faces.  One lane per point.  It drops the body when
 *   its box, grown by the radius, misses the query, and otherwise walks the grid in rings of cells
 *   around the cell of the query clamped into the box, nearest ring first, until a conservative lower
 *   bound on the distance to every cell not yet visited exceeds the best D2; inside a ring a cell
 *   whose own bound exceeds it is skipped (csrc/mh_surface.hip argues the bounds and their margin:
 *   pruned only on strictly greater, so a tie with a smaller face index survives).  Every trip count is bounded by the grid's dimensions, never by
 *   a distance: a query 1000 m away with radius = +inf costs one pass over the body's cells.
 *   d2, face (B,Q), point, weights (B,Q,3): each may be NULL, not all.
 *   Refused before any HIP call: B, V, F or Q <= 0; B Q or 16 B F beyond one launch; NULL faces, ws or
 *   points; every output NULL; a radius that is NaN, <= 0 or -inf (+inf is allowed).
 * mh_person_surface: verts (T,N,V,3), and ws as mh_surface_grid filled it for THE SAME verts taken as
 *   B = T N bodies; mask (T,N,V) uint32 as mh_person_inside wrote it for them, or NULL (nobody is
 *   inside anybody).  One lane per vertex v of a live person n with three finite coordinates, which
 *   walks the other live bodies m != n of its frame:
 *     bit m of the mask set: body m is searched with an UNBOUNDED radius and without the box test (the
 *       vertex is in m's box, the walk ends after a few rings), so that every penetrating vertex gets
 *       a depth, however deep it is;
 *     otherwise: body m is searched with radius.
 *       out_d2, out_idx = over the bodies that do NOT contain the vertex, the smallest D2 and
 *                         m F + f of its face; on a tie the smallest m, then the smallest f;
 *       in_d2, in_idx   = over the bodies that CONTAIN it, the LARGEST of its D2 to each body's
 *                         surface (the body it is deepest in) and m F + f; on a tie the smallest m;
 *       out_pt, in_pt (T,N,V,3) = the closest points themselves, zeros where there is none;
 *       stats (T,N,V,2) int32 = bodies searched (not dropped at their box) and faces evaluated: what
 *                         the measurements in DESIGN.md are made of.
 *   Without a candidate (and for a dead person or a query that is not finite) D2 = +inf, idx = -1.
 *   Every output is overwritten; each may be NULL, not all.
 *   Refused before any HIP call: T, N, V or F <= 0; N > 32; N F >= 2^31; T N V or 16 T N F beyond one
 *   launch; NULL faces, ws or verts; every output NULL; a radius that is NaN, <= 0 or -inf.
 * mh_surface_pairs: out_d2, out_idx, in_d2, in_idx (T,N,V) as mh_person_surface wrote them; part (V)
 *   uint8; P <= 32 parts; contact in metres, finite, >= 0; c2 = contact contact (float32).
 *       pair_depth_d2[t][n][m] = the largest in_d2 over the vertices of n with in_idx / F = m,
 *                                -1 when there is none;
 *       pair_min_d2[t][n][m]   = the smallest out_d2 over the vertices of n with out_idx / F = m,
 *                                +inf when there is none;
 *       pair_contact[t][n][m]  = the number of those vertices with out_d2 <= c2;
 *       part_depth_d2, part_min_d2, part_contact (T,N,P): the same three over the vertices with
 *                                part[v] = k, whatever the other body.
 *   A part[v] >= P counts in no part; an idx at or beyond N F is treated as idx < 0; a d2 that is NaN or
 *   negative is never a minimum or a maximum.  Integer atomics only -- counts, and minima and maxima on
 *   the BIT PATTERN of non-negative floats -- accumulated in LDS per workgroup, then one atomic per
 *   workgroup and accumulator in device memory, as mh_person_pairs does it; V need not be a multiple
 *   of the workgroup.  Every output is overwritten; each may be NULL, not all.
 *   Refused before any HIP call: T, N, V or F <= 0; N > 32; P outside 1..32; N F >= 2^31; T N V beyond
 *   one launch; NULL out_d2, out_idx, in_d2, in_idx or part; every output NULL; a contact that is not
 *   finite or is negative.
 * The calls own nothing and keep nothing beyond the switch of mh_surface_set_all_faces.               */
size_t mh_surface_grid_bytes(int B, int F);
int mh_surface_grid(int B, int V, int F, const float* verts /*(B,V,3)*/, const int32_t* faces /*(F,3)*/,
                    const uint8_t* live /*(B)*/, void* ws, size_t ws_bytes, int32_t* status /*(B)*/,
                    void* stream);
int mh_surface_set_all_faces(int on);
int mh_mesh_closest(int B, int V, int F, const int32_t* faces, const void* ws, int Q,
                    const float* points /*(B,Q,3)*/, float radius, float* d2 /*(B,Q)*/,
                    int32_t* face /*(B,Q)*/, float* point /*(B,Q,3)*/, float* weights /*(B,Q,3)*/,
                    void* stream);
int mh_person_surface(int T, int N, int V, int F, const int32_t* faces, const void* ws,
                      const float* verts /*(T,N,V,3)*/, const uint32_t* mask /*(T,N,V)*/, float radius,
                      float* out_d2, int32_t* out_idx, float* in_d2, int32_t* in_idx /*(T,N,V)*/,
                      float* out_pt, float* in_pt /*(T,N,V,3)*/, int32_t* stats /*(T,N,V,2)*/,
                      void* stream);
int mh_surface_pairs(int T, int N, int V, int F, const float* out_d2, const int32_t* out_idx,
                     const float* in_d2, const int32_t* in_idx, const uint8_t* part /*(V)*/, int P,
                     float contact, float* pair_depth_d2 /*(T,N,N)*/, float* pair_min_d2 /*(T,N,N)*/,
                     int32_t* pair_contact /*(T,N,N)*/, float* part_depth_d2 /*(T,N,P)*/,
                     float* part_min_d2 /*(T,N,P)*/, int32_t* part_contact /*(T,N,P)*/, void* stream);

/* ---- stand-alone forms of losses.py:19-40 and morphology.py:6-41 (call compatibility of
 * mhmocap.losses / mhmocap.morphology; the optimiser uses the fused kernels above) --------------
 * mh_avg_depth_loss: rows = b*N maps of P pixels; `tru` has rows/group maps (group = N when the
 * target is (b,1,H,W)).  row_sums (rows,3) = {sum m*log(clamp pred), sum m*log(clamp true), sum m};
 * the loss is sum_r ((s0 - s1)/(s2+1))^2, which the host forms from row_sums.  row_loss must not be NULL but is
 * neither read nor written (it may be row_sums itself): nothing on the device evaluates the per-row loss.
 * _backward: gpred (rows,P), gtrue_rows (rows,P) [caller sums the group], scaled by grad_out.      */
int mh_avg_depth_loss(const float* pred, const float* tru, const float* mask, int rows, int group,
                      size_t P, float eps, float* row_sums, float* row_loss, void* stream);
int mh_avg_depth_loss_backward(const float* pred, const float* tru, const float* mask, int rows,
                               int group, size_t P, float eps, const float* row_sums,
                               float grad_out, float* gpred, float* gtrue_rows, void* stream);
/* sums2 = { sum((mask*(a-b))^2), sum(mask) }; loss = sums2[0] / (sums2[1] + 1)                     */
int mh_masked_mse(const float* a, const float* b, const float* mask, size_t n, float* sums2, void* stream);
int mh_masked_mse_backward(const float* a, const float* b, const float* mask, size_t n,
                           const float* sums2, float grad_out, float* ga, void* stream);
/* binary erosion (dilate = 0) / dilation (dilate = 1) with a k x k window of ones on float maps    */
int mh_morph_f32(const float* in, float* out, int n_images, int H, int W, int kernel_size,
                 int dilate, void* stream);

/* generic forms of camera_projection_torch / camera_inverse_projection_torch (transforms.py:57-95,
 * 114-130): pts (B,M,3), K_dev (B,3,3) DEVICE, Kd_host 5 HOST coefficients or NULL;
 * out (B,M,2) or (B,M,3) with the depth appended (return_depth).                                 */
int mh_project_points(int B, int M, const float* pts, const float* K_dev, const float* Kd_host,
                      int with_depth, float* out, void* stream);
int mh_unproject_points(int B, int M, const float* uvd, const float* K_dev, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MHMOCAP_HIP_H */
