// Host-side objects behind the opaque C handles.
#pragma once
#include <mutex>

#include "common.h"
#include "gemm.h"

struct mi_pool;   // pool.hip (include/matinvent_hip_pool.h): the memory behind a pooled batch handle

struct ParamInfo {
    std::string name;
    int64_t off, numel;
    int rows, cols;
};

struct mi_net {
    mi_net_config cfg;
    int H, L, F, TD, KP, NT;  // KP = 3*FP (sin,cos) pairs, FP = F rounded up to 8; NT = H/32
    int edge_in;              // 2H + 9 + 6F
    int Z = 0, lat_P = 0, lat_F = 0;   // property part of the embedding input (guidance.hip, mi_net_set_latent): the last Z = 2 lat_F lat_P of the TD columns; 0: none
    std::vector<ParamInfo> params;
    int64_t nparams = 0;
    const float* theta = nullptr;  // caller-owned flat parameters (device)
    uint64_t param_epoch = 0;      // bumped by every mi_net_set_params: what an evaluation left behind for a later one (mi_batch::G, PQ0) is valid for ONE parameter version
    float* freqs = nullptr;        // [F] device
    bool have_freqs = false;
    // packed copies, rebuilt by mi_net_set_params
    float* Whh = nullptr;    // [L][2H][H]   rows [0,H) = W1[:, :H], rows [H,2H) = W1[:, H:2H]
    float* Wff_p = nullptr;  // [L][KP/4][NT][64][4]
    float* W2_p = nullptr;   // [L][NT][NT][4][64][4]
    float* Wff = nullptr;    // [L][H][6F]  Fourier column block of edge_mlp.0, contiguous (GEMM edge path)
    int edge_mode = 1;       // MI_EDGE_GEMM (default) or MI_EDGE_FUSED_F32
    unsigned short* Wffpl = nullptr;  // [L][3][H][ld(6F)] bf16 planes of Wff
    unsigned short* W2pl = nullptr;   // [L][3][H][H]      bf16 planes of edge_mlp.2.weight
    // [L] plane sets of the node-level weights, grouped by the operand they multiply:
    unsigned short* Wlnpl = nullptr;   // (3H x H): [P_i block; P_j block; node_mlp.0.weight[:, :H]] -- everything LayerNorm(h) feeds
    unsigned short* Waggpl = nullptr;  // (H x H):  node_mlp.0.weight[:, H:]  (multiplies the aggregated messages)
    unsigned short* Wn2pl = nullptr;   // (H x H):  node_mlp.2.weight
    unsigned short* Wffc = nullptr;    // [L] the pair-layout Fourier block of edge_mlp.0 in MFMA fragment order (edge_stage.hip: first edge GEMM)
    unsigned short* Wnc = nullptr;     // [L] the three operands above in MFMA fragment order: [Wagg | Wn2 | Wln] (node_chain.hip; H = 128 / 256 / 512 with LayerNorm)
    float* wbounds = nullptr;          // [L][8] row-sum / bias bounds of the layer's weights (fp16 plane format: activation scales)
    // pair mode of the first edge GEMM (symmetric edge lists): K' = 2*Kh columns = [sin block | pad | cos block | pad],
    // Kh = 3F rounded up to 32, so that each block is a whole number of k-tiles
    int Kh = 0;
    unsigned short* Wffpl_pair = nullptr;  // [L] plane sets of the Fourier block of edge_mlp.0 in that column layout
    float* C0 = nullptr;                   // [L][H] sum of the cosine-block weights = the Fourier term of a self edge (d = 0)
    // transposed copies for the data-gradient GEMMs (training), rebuilt with the packs
    float* W2T = nullptr;    // [L][H][H]
    unsigned short* W2Tpl = nullptr;  // [L] plane sets of W2T (fp16 plane format): the W operand of the dM1 data gradient
    unsigned short* W2Tf = nullptr;   // [L] the same in MFMA fragment order (Planes::frag: the register-tile GEMM, hidden_dim % 256 == 0)
    float* Wn2T = nullptr;   // [L][H][H]
    float* Wn1T = nullptr;   // [L][2H][H]
    float* WhhT = nullptr;   // [L][H][2H]
    float* WaT = nullptr;    // [H][H]   (atom_latent_emb.weight[:, :H])^T
    unsigned short* Wbw = nullptr;   // [L] fragment-order packs of the TRANSPOSED node-level weights [WhhA | WhhB | Wn2^T | Wn0^T]: the fused backward chain (node_bwd.hip)
    float* WheadT = nullptr; // [H][104] coord_out.weight (3 rows) and type_out.weight (100 rows) transposed side by side (inference heads)
    // profiling of the dominant kernel (event pairs; launches may come from several host threads / streams)
    bool prof = false;
    std::vector<hipEvent_t> ev;  // pairs
    size_t ev_used = 0;
    hipEvent_t ev_origin = nullptr;
    std::mutex prof_mu;

    int64_t off(const std::string& name) const;
    const float* p(const std::string& name) const { return theta + off(name); }
    size_t whh_stride() const { return (size_t)2 * H * H; }
    size_t wff_stride() const { return (size_t)(KP / 4) * NT * 256; }
    size_t w2_stride() const { return (size_t)NT * NT * 4 * 256; }
};

// Saved activations of one training forward + backward scratch (allocated on first use).
struct Tape {
    bool allocated = false, valid = false;
    float *cat = nullptr, *Z1 = nullptr, *Z2 = nullptr, *Xpre = nullptr, *Ypre = nullptr, *lnstat = nullptr, *gf = nullptr;
    float *atom_types = nullptr, *t_emb = nullptr, *lattices = nullptr, *frac = nullptr;
    // what the backward reads of the forward's INPUTS: the tape's copies above (mi_cspnet_forward_train: the caller may overwrite its arrays before the
    // backward), or -- `borrow_inputs`, set by the fused micro-step around its own training forward -- the caller's arrays themselves (they are the
    // tape's noised inputs and the batch's time embedding, alive until the micro-step's backward has run: four copy launches fewer per micro-step)
    const float *in_types = nullptr, *in_temb = nullptr, *in_lat = nullptr, *in_frac = nullptr;
    bool borrow_inputs = false;
    float *dh = nullptr, *dY = nullptr, *dXa = nullptr, *Xa = nullptr, *dcat = nullptr, *dPQ = nullptr, *dG = nullptr, *dgf = nullptr,
          *dlo = nullptr, *dtproj = nullptr, *M1 = nullptr, *dM1 = nullptr, *FF = nullptr, *scratch = nullptr;
    // fused fine-tune micro-step: noised inputs, targets, gradient seeds, per-crystal losses
    float *nz_lat = nullptr, *nz_frac = nullptr, *nz_types = nullptr, *tar_x = nullptr, *rnd_l = nullptr, *rnd_t = nullptr, *d_l = nullptr,
          *d_x = nullptr, *d_t = nullptr, *Lb = nullptr, *KLb = nullptr;
    float* lnpart = nullptr;      // [L][ceil(N / 32)][2H] per-workgroup partial sums of d ln_w | d ln_b of the fused backward chain (node_bwd.hip), reduced for all layers at once
    float* dsc_layers = nullptr;  // [L][8] each layer's activation scales of the training forward (fp16 plane format, folded launch)
    // fp16 plane format: every layer's M1 plane set of the training forward, kept for edge_mlp.2's weight gradient (gemm_tn_planes, backward.hip:
    // the product reads both operands as the plane sets their producers wrote instead of re-splitting -- and re-evaluating SiLU on -- fp32 rows)
    unsigned short* M1pl_l = nullptr;
    size_t m1pl_stride = 0;       // elements per layer
    // and the pair differences / sums of dZ1 (the A operands of the Fourier block's weight gradient) as plane sets, written by the fused pair pass
    unsigned short *DmPl = nullptr, *DpPl = nullptr;
    bool dsc_layers_valid = false;
    size_t scratch_floats = 0;
    // Deferred node-level weight gradients (mi_batch_set_wgrad_window).  Between two optimizer steps the weights do not change, so the
    // weight gradient of a node-level linear over `wslots` micro-steps is ONE contraction over wslots x N rows instead of wslots
    // contractions over N rows (N = 1.7k atoms per crystal group: 24 launches of ~20 us plus as many partial reductions per evaluation,
    // each leaving most of the chip idle).  The operand pairs of every layer are kept per micro-step, slot after slot, rows contiguous:
    //   w_dY | w_Xa  -> node_mlp.2.weight / bias      w_dXa | w_cat -> node_mlp.0.weight / bias      w_dPQ | w_cat[:, :H] -> edge_mlp.0.weight[:, :2H]
    // layout [L][wslots x N][width]; the training forward writes its `cat` rows straight into slot `wcur`, the backward its dY / Xa / dXa /
    // dPQ; net_wgrad_flush contracts rows 0 .. wcur x N and resets wcur (automatically when the window is full).
    int wslots = 0, wcap = 0, wcur = 0;
    float *w_dY = nullptr, *w_Xa = nullptr, *w_dXa = nullptr, *w_cat = nullptr, *w_dPQ = nullptr;
    // ... and (round 6) the HEAD and EMBEDDING weight gradients in the same window -- six short contractions + three column sums per micro-step, each with its
    // own partial reduction (18 launches), become the same nine over wslots x the rows.  Their operand rows, layout [wslots][rows][width], slot `wcur`:
    //   w_dlo [B,12] | w_gf [B,H] -> lattice_out.weight      w_dtype [N,100] | w_hf [N,H] -> type_out.weight / bias      w_dcoord [N,3] | w_hf -> coord_out.weight
    //   w_dh [N,H] | w_x1 [N,H] -> atom_latent_emb.weight[:, :H] / bias      w_dtproj [B,H] | w_temb [B,TD] -> atom_latent_emb.weight[:, H:]
    //   w_eXa [N,H] | w_types [N,100] -> node_embedding.weight / bias
    // The training forward and the backward write them IN PLACE: while a window is open, the batch's x1 / hf, the tape's gf / dlo / dtproj / d h and the
    // micro-step's noised types, time embedding and gradient seeds LIVE in the slot (the pointer accessors below); nothing is copied on the fused route.
    float *w_dlo = nullptr, *w_gf = nullptr, *w_dtype = nullptr, *w_dcoord = nullptr, *w_hf = nullptr, *w_dh = nullptr, *w_x1 = nullptr, *w_dtproj = nullptr,
          *w_temb = nullptr, *w_eXa = nullptr, *w_types = nullptr;
    bool head_window() const { return wslots > 0 && w_hf != nullptr; }
};

struct mi_batch {
    int B = 0, N = 0, H = 0, L = 0;
    int64_t E = 0;      // edges of the current graph (fixed for fc; rewritten by every forward for knn)
    int64_t E_cap = 0;  // edge capacity every per-edge buffer is sized for (= E for fc)
    const int* e_dev = nullptr;   // knn lists rebuilt WITHOUT a host round trip (knn_build nosync): E above is the capacity the launches are sized for, *e_dev the edge count
    int64_t e_hint = 0;           // the last edge count the HOST has seen (a synchronising build, mi_knn_graph_status): picks kernel forms for capacity-sized launches
    bool knn_nosync = false;      // set by mi_sampler_run around its forwards: the chain's graph builds do not synchronise (mi_knn_graph_status reads the verdict behind it)
    int nslots = 1;
    int seg_shift = 5;  // log2 of the row-block size behind the partial sums currently in `part` (5: plane GEMM epilogue; 7: edge_stage.hip)
    // knn edge style (CSPNet.gen_edges knn branch, graph.hip)
    int knn = 0, max_neighbors = 0, cap_per_node = 0, deg_cap = 0, nmax = 0;
    // pair tables of the fc edge list (unordered node pairs i < j of each crystal): the first edge GEMM runs over pairs
    int64_t Np = 0;
    int *pair_i = nullptr, *pair_j = nullptr, *pair_e1 = nullptr /*edge i->j*/, *pair_e2 = nullptr /*edge j->i*/, *pair_graph = nullptr,
        *e_diag = nullptr /*[N] self edge of node i*/;
    int* pair_off = nullptr;  // [B+1] first pair row of each crystal (fc list); nmax_fc = largest atom count
    int nmax_fc = 0;
    float* fd = nullptr;    // [E][3] explicit frac_diff per edge (CSR order); nullptr = fc: (x_dst - x_src) % 1
    int* inedge = nullptr;  // [E] edge ids grouped by destination node, node v at rowptr[v]..rowptr[v+1] (degrees are symmetric)
    int *kn_ent = nullptr, *kn_acnt = nullptr, *kn_deg = nullptr, *kn_mcount = nullptr, *kn_eoff = nullptr, *kn_meta = nullptr,
        *kn_refpos = nullptr, *r_src = nullptr, *r_dst = nullptr;
    float* r_vec = nullptr;  // reference-order copy of the list: edges (r_src, r_dst), attribute r_vec
    int64_t node_offset = 0, graph_offset = 0;
    std::vector<int> num_atoms_h, node_off_h;
    // index tables (device)
    int *num_atoms = nullptr, *node_off = nullptr /*[B+1]*/, *node2graph = nullptr, *src = nullptr, *dst = nullptr,
        *rowptr = nullptr /*[N+1]*/, *edge_graph = nullptr /*[E]*/;
    // forward workspace (device)
    float *x1_base = nullptr, *hf_base = nullptr;   // the handle's own x1 / hf buffers (x1 / hf point into the weight-gradient window's slot while a training forward with an open window runs)
    float* h = nullptr;      // [L+1][N][H] node features before layer l / after the last
    float* cat = nullptr;    // [N][2H]  (LN(h) | agg)
    float* PQ = nullptr;     // [N][2H]
    float* PQ0 = nullptr;    // layer 0's [P_i | P_j | X_part] of the INFERENCE node chain, in a buffer of its own: the sampler's predictor evaluation starts from
                             // the same embedding as the corrector evaluation in front of it, so layer 0's LayerNorm + projections launch is not repeated (pq0_valid)
    bool pq0_valid = false;
    const void* reuse_net = nullptr;   // the network whose evaluation left G / PQ0 behind (another network's evaluation never reuses them)
    uint64_t reuse_epoch = 0;          // ... and its parameter version (mi_net::param_epoch): an optimizer step in between invalidates both
    float* G = nullptr;      // [B][H]
    float* part = nullptr;   // [nslots][N][H]
    float* FFp = nullptr;    // [tiles][KP/4][64][4] Fourier operand, B-fragment order (fused path)
    float* FF = nullptr;     // [E][6F] Fourier features, reference column order (GEMM path)
    float* M1 = nullptr;     // [E][H]
    float* M2 = nullptr;     // [E][H]
    unsigned short* FFpl = nullptr;  // [3][E][ld(6F)] bf16 planes of the Fourier features
    unsigned short* M1pl = nullptr;  // [3][E][H]      bf16 planes of M1
    unsigned short* m1_cur = nullptr;  // the plane set this layer's edge products write / read: M1pl, or the layer's slot of Tape::M1pl_l in a training forward
    unsigned short* lnpl = nullptr;  // plane sets of LayerNorm(h) and of the aggregated messages (N x H each)
    unsigned short* aggpl = nullptr;
    unsigned short* Xpl = nullptr;   // plane set of the node MLP's hidden activation (N x H)
    float* dsc = nullptr;            // [6][2] {scale, 1/scale}: this layer's M1 / agg / X plane sets; backward pass: dZ2, the pair differences, the Fourier features (fp16 plane format)
    unsigned* absmax = nullptr;      // [2 L] bit patterns: [2l] = max |P_i, P_j, X_part| of layer l, [2l + 1] = max |G[l]| (zeroed per evaluation); [2L], [2L + 1] = max |d cat|, max |dM1| of the layer the backward pass is in
    int* e2_tab = nullptr;           // per-tile tables of the second edge GEMM (edge_stage.hip: EG2_TAB ints per 128-row tile), valid for graph_epoch == e2_tab_epoch
    bool gram_valid = false;         // b->G and its absmax slots hold the lattice term of the previous (inference) evaluation of this handle
    bool ff_built_once = false;      // (timing ablation mi_debug_set_skip bit 4 only: the Fourier operand exists)
    int e2_tab_epoch = -1, graph_epoch = 0;   // graph_epoch: bumped whenever the edge list changes (knn: every forward)
    unsigned* nc_flags = nullptr;    // [L + 1][2 x row blocks] arrival counters of node_cols_kernel's in-launch hand-overs (zeroed per evaluation)
    float* X = nullptr;      // [N][H] node-MLP hidden
    float* x1 = nullptr;     // [N][H] node_embedding output
    float* tproj = nullptr;  // [B][H]
    float* hf = nullptr;     // [N][H] after the final LayerNorm
    // sampler scratch
    float* temb = nullptr;     // [B][TD]
    int* times = nullptr;      // [B]
    float* pred_l = nullptr;   // [B][9]
    float* pred_x = nullptr;   // [N][3]
    float* pred_t = nullptr;   // [N][100]
    float* x_mid = nullptr;    // [N][3]
    float* lp_corr = nullptr;  // [B]
    float* coef = nullptr;     // [T+1][MI_NCOEF]
    int coef_T = -1;
    std::vector<float> coef_h;  // host copy of what `coef` holds (re-uploaded only when the caller's table differs)
    int keep_lattice = 0, keep_coords = 0;  // CSP mode of the sampler (mi_sampler_set_keep)
    mi::SplitK sk;  // split-K scratch of the node-level products (small batches only)
    // optional helper stream of higher priority for the node-level kernels of an inference forward (see net_forward) + its join events
    hipStream_t hi_stream = nullptr;
    hipEvent_t hi_ev[2] = {nullptr, nullptr};
    Tape tape;
    uint64_t fwd_epoch = 0;   // bumped by every evaluation of this handle (net_forward): what a pending backward's caller saw must still be current
    // mi_traj_logprob (traj_logprob.hip): the local derivatives of the last taped call that used this handle -- d log_prob / d(network output),
    // per element, before the upstream gradient -- and the gradient seeds its backward hands to net_backward (allocated on first use)
    float *tr_dl = nullptr, *tr_dx = nullptr, *tr_dt = nullptr;      // [B][9], [N][3], [N][A]
    float *tr_sl = nullptr, *tr_sx = nullptr, *tr_st = nullptr;      // the seeds, same shapes
    mi_batch* tr_partner = nullptr;                                   // (corrector handle) the predictor handle of that call; NULL: no taped call pending
    uint64_t tr_epoch = 0, tr_partner_epoch = 0;                      // both handles' fwd_epoch right after that call
    // mi_traj_pg_step (corrector handle): the gathered state at t and t-1, the new log-probabilities and their seeds (allocated on first use)
    float *pg_a = nullptr, *pg_x = nullptr, *pg_xm = nullptr, *pg_l = nullptr;     // [N][A], [N][3], [N][3], [B][9]
    float *pg_na = nullptr, *pg_nx = nullptr, *pg_nl = nullptr;                    // [N][A], [N][3], [B][9]
    float *pg_lp = nullptr, *pg_g = nullptr;                                       // [3][B] each
    int* pg_t = nullptr;                                                           // [B] the times the kernels read (checked copy)
    // mi_traj_pg_kl_step (allocated on first use).  Corrector handle: d KL_k / d(agent output) of the last call and the per-term KL when the
    // caller keeps none.  Prior handle: the prior's corrector coordinate head (its predictor's heads stay in pred_l / pred_x / pred_t).
    float *kl_dl = nullptr, *kl_dt = nullptr, *kl_dxc = nullptr, *kl_dxp = nullptr;   // [B][9], [N][A], [N][3], [N][3]
    float* kl_val = nullptr;                                                            // [3][B]
    float* kl_pxc = nullptr;                                                            // [N][3] (prior handle)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;  // fork / join of work put on an auxiliary stream (mi_ft_micro_step)
    // strided reverse chain (stride.hip, mi_batch_set_time_map): step index k -> trained time tau_k, read by the time embedding alone
    int* time_map = nullptr;       // [time_map_h.size()] device; NULL: no map, the step index is the time
    int* time_map_buf = nullptr;   // its allocation (kept when the map is cleared)
    int time_map_cap = 0;
    std::vector<int> time_map_h;   // host copy: length checks, comparison between handles
    // replacement conditioning (condition.hip, mi_batch_set_condition): masks, clean values and the level table on the device
    bool cond_on = false;          // a condition is attached (mi_sampler_run imposes it; false: the chain's launches are those of before)
    bool cond_any = false;         // ... and at least one element is known (nothing known: no launch)
    int cond_levels = 0;           // rows of cond_table (= T + 1 of the chains it is for)
    int cond_table_cap = 0;
    int *cond_kt = nullptr, *cond_kx = nullptr, *cond_kl = nullptr, *cond_types0 = nullptr;   // [N], [N], [B], [N] (allocated on first use)
    float *cond_frac0 = nullptr, *cond_lat0 = nullptr, *cond_table = nullptr;                  // [N][3], [B][9], [cond_levels][3]
    bool cond_has_x = false, cond_has_l = false;   // ... a coordinate / a lattice among the known (what a symmetry constraint refuses)
    // likelihood mask (condition.hip, mi_batch_set_likelihood_mask): the elements whose predictor terms leave the trajectory
    // likelihood -- state of its own, apart from the condition above (a policy-gradient handle carries the masks alone)
    bool lik_on = false;
    int *lik_kt = nullptr, *lik_kx = nullptr, *lik_kl = nullptr;      // [N], [N], [B] 0 / 1 (allocated on first use)
    std::vector<int> lik_h;                                           // host copy [N | N | B]: comparison between the handles of a call
    // resampling jumps of a conditioned chain (resample.hip, mi_batch_set_resampling): r visits per jump-off level, jumps of j
    // levels, and the jump table on the device
    bool rs_on = false;
    int rs_r = 1, rs_j = 0;
    int rs_levels = 0;             // rows of rs_table (= T + 1 of the chains it is for)
    int rs_table_cap = 0;
    float* rs_table = nullptr;     // [rs_levels][3] = (c0, c1, s) of the jump a -> a + j; rows with a + j > T are zero
    // preference pairs (dpo.hip, mi_batch_set_pairs): (winner, loser) crystal indices, and per crystal the list of its pair slots in
    // ascending pair index -- entry 2 p: crystal is pair p's winner, 2 p + 1: its loser
    int n_pairs = 0, pairs_cap = 0;
    int *dpo_w = nullptr, *dpo_l = nullptr;          // [n_pairs]
    int *dpo_off = nullptr, *dpo_slots = nullptr;    // [B + 1], [2 n_pairs]
    float* dpo_delta = nullptr;                      // [B]: d_b
    float *dpo_m = nullptr, *dpo_g = nullptr;        // [n_pairs]: m_p, g_p
    std::vector<int> dpo_w_h, dpo_l_h;
    // supervised training micro-step (pretrain.hip, mi_pretrain_micro_step; allocated on first use): the crystals' schedule rows, their
    // sums of squares, and -- forward-only form, which prepares no tape -- the noised inputs and targets
    float *pt_sched = nullptr, *pt_parts = nullptr;   // [B][4], [B][3]
    float* pt_noised = nullptr;                       // in_lat | in_frac | in_types | tar_x | rnd_l | rnd_t
    // pooled handle (pool.hip, mi_batch_create_pooled): the pool every buffer above was lent by (NULL: the handle owns them),
    // the two prefix arrays next to node_off_h that the index-table kernels read, and the device copy of the edge prefix
    // supervised training with a condition (guidance.hip, mi_pretrain_micro_step_cond; allocated on first use): the crystals' dropout draws
    int* gd_drop = nullptr;                           // [B] 0 / 1
    // classifier-free guidance (guidance.hip, mi_batch_set_guidance): the crystals' normalised properties, the frequency table and the
    // handle the null evaluation runs on
    bool gd_on = false;
    int gd_P = 0, gd_F = 0, gd_cap = 0;
    float gd_gamma = 0.f;
    mi_batch* gd_partner = nullptr;
    float *gd_yhat = nullptr, *gd_freqs = nullptr;    // [B][gd_P], [MI_GUIDANCE_MAX_FREQS]
    int* gd_have = nullptr;                           // [B][gd_P]
    // property predictor (scalar_head.hip, include/matinvent_hip_scalar.h; allocated on first use): the clean network inputs of the
    // inference form (the taped form keeps them in the tape), the pooled features, and for sc_P properties the seeds d out and the crystals' loss terms
    float* sc_in = nullptr;                           // in_lat [B][9] | in_frac [N][3] | in_types [N][100]
    float *sc_gf = nullptr, *sc_dout = nullptr, *sc_parts = nullptr;   // [B][H], [B][sc_P], [B][sc_P][3] = e^2, |e|, present
    int sc_P = 0, sc_last_P = 0;                      // the per-property buffers' capacity; the P of the last call (their layout)
    // predictor-steered sampling (steer.hip, include/matinvent_hip_steer.h; allocated on first use): the noised micro-step's schedule
    // rows and -- forward-only form, which prepares no tape -- the noising's three by-products; the resampling's per-group flags and ESS
    float *st_sched = nullptr, *st_noise = nullptr;   // [B][4]; tar_x [N][3] | rnd_l [B][9] | rnd_t [N][100]
    float* st_parts = nullptr;                        // [B][2] = (flags, ESS) of group g in row g (B rows: room for K = 1)
    // input gradient of the predictor (input_grad.hip, include/matinvent_hip_inputgrad.h; allocated on first use): the pairs'
    // d u / d Delta summed over the layers, and the transposed Fourier columns of every layer's edge_mlp.0.weight (the W operand of gemm_nt)
    // with the network and parameter version they were packed from
    float* ig_dd = nullptr;                           // [Np][3]
    float* ig_wT = nullptr;                           // [L][6F][H]
    const void* ig_net = nullptr;
    uint64_t ig_epoch = 0;
    // symmetry constraint (sym_constraint.hip, mi_batch_set_symmetry): per crystal the operation count and the distinct rotation
    // parts, per atom the orbit representative and the affine map from its coordinates; the failure counters of the cell projection
    bool symc_on = false;          // a constraint is attached (mi_sampler_run imposes it; false: the chain's launches are those of before)
    bool symc_any = false;         // ... and at least one crystal has more than the identity (none: no launch)
    int symc_rot_cap = 0;
    int *symc_K = nullptr, *symc_roff = nullptr, *symc_rot = nullptr, *symc_rep = nullptr, *symc_fail = nullptr;   // [B], [B + 1], [roff[B]][9], [N], [B]
    double *symc_Q = nullptr, *symc_d = nullptr;                                                                    // [N][9], [N][3]
    mi_pool* pool = nullptr;
    std::vector<int> edge_off_h, pair_off_h;
    int* edge_off = nullptr;   // [B + 1] first edge of each crystal (pooled handles only)
    std::vector<void*> allocs;
};

namespace mi {
// reuse_embedding -- the CONTRACT (internal; the only caller is mi_sampler_run's predictor evaluation, diffusion.py:320-322): this evaluation has the same
// t_emb, atom_types AND lattices as the previous evaluation of this batch handle by this network at this parameter version; only the coordinates moved.
// It keeps h[0], and (inference, pair mode) the lattice term G of every layer and layer 0's [P_i | P_j | X_part].  The handle remembers the network and
// its parameter epoch, so another network or an mi_net_set_params in between falls back to recomputing G / PQ0; unchanged lattices are the caller's promise.
int net_forward(mi_net* net, mi_batch* b, const float* t_emb, const float* atom_types, const float* frac,
                const float* lattices, float* lattice_out, float* coord_out, float* type_out, hipStream_t s, bool train = false,
                bool reuse_embedding = false, bool coords_only = false, bool trunk_only = false);
int net_tape_prepare(mi_net* net, mi_batch* b);
int net_pack_transposes(mi_net* net, hipStream_t s);
// dgf_seed [B][H] (scalar_head.hip): the pass is seeded from d gf ALONE -- d hf[i] = dgf_seed[g(i)] / n_g, no head's backward, the lattice_out.* /
// type_out.* / coord_out.* slices of `grad` untouched; d_lat / d_coord / d_type are not read.  NULL: the three heads' seeds, as ever.
// ig (input_grad.hip): the DATA-ONLY, input-gradient form -- `grad` is NULL and never read: no weight-gradient contraction or
// reduction is launched, and the pass additionally produces d / d(coordinates, lattices, type rows) of what seeded it.  Pair mode only (its
// entry refuses everything else).  NULL: the pass of before, launch for launch.
struct InputGradOut {
    float *g_types, *g_frac, *g_lat;   // [N][100] or NULL, [N][3], [B][9]
};
int net_backward(mi_net* net, mi_batch* b, const float* d_lat, const float* d_coord, const float* d_type, float* grad, hipStream_t s,
                 const float* dgf_seed = nullptr, const InputGradOut* ig = nullptr);
// input_grad.hip: the new launches of that form.  input_grad_pairs: d Delta (b->ig_dd) (=, when `first`, else +=) the chain rule through
// sin / cos of dSC [Np][6F] = [Dm Wsin | Dp Wcos]; input_grad_finish: the scatter to the atoms, the lattice term's chain rule over t.dG
// and (g_types) dXa node_embedding.weight.
int input_grad_prepare(mi_net* net, mi_batch* b, hipStream_t s);   // the handle's buffers of this form and the transposed Fourier columns (once per parameter version)
int input_grad_pairs(mi_net* net, mi_batch* b, const float* frac, const float* dSC, bool first, hipStream_t s);
int input_grad_finish(mi_net* net, mi_batch* b, const InputGradOut* ig, const float* lattices, const float* dG, const float* dXa, hipStream_t s);
// scalar_head.hip: that broadcast (one launch), and the trunk's forward alone -- net_forward(trunk_only) ends behind the final LayerNorm, b->hf
int scalar_seed_hf(const mi_batch* b, const float* dgf, float* dhf, int H, hipStream_t s);
// scalar_head.hip: the body of the predictor's entries with the INPUT STAGE passed in (steer.hip: the noised micro-step, the forward on a
// chain state).  The stage runs behind every host-side check and the buffers' allocation; it fills b->temb [B][TD] and either writes the
// network inputs into w_lat / w_frac / w_types (the tape's noised-input arrays when `train`, the handle's sc_in otherwise) or -- a stage
// that reads the caller's arrays, own_inputs: nothing is allocated for it, the three w_* are NULL -- points in_* at them.  stage == NULL:
// the clean inputs of (lengths, angles, frac0, atom_types) at `times` / t_all, as ever.
struct ScalarStageIO {
    float *w_lat, *w_frac, *w_types;
    const float *in_lat, *in_frac, *in_types;
    bool train;
};
typedef int (*scalar_input_stage_fn)(mi_net* net, mi_batch* b, ScalarStageIO* io, void* ctx, hipStream_t s);
int scalar_run(const char* what, mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
               const float* time_freqs, const int* times, int t_all, const float* W, const float* bias, int P, const float* yhat, const int* have,
               const int* have_host, const int* count_global, const int* count_global_host, int accum_steps, int loss_kind, float* grad_theta,
               float* grad_W, float* grad_bias, float* stats, float* out, void* stream, scalar_input_stage_fn stage = nullptr,
               void* stage_ctx = nullptr, bool own_inputs = false, const float* ig_dout = nullptr, const InputGradOut* ig = nullptr);
// steer.hip: the input stage of a chain STATE (the caller's arrays are the network inputs; the stage fills the time embedding alone)
struct ScalarStateCtx {
    const float *atom_types, *frac, *lattices, *time_freqs;
    const int* times;
    int t_all;
};
int scalar_state_stage(mi_net* net, mi_batch* b, ScalarStageIO* io, void* ctx, hipStream_t s);
// backward.hip: the fine-tune micro-step's sequence -- time fill and embedding, add_noise_kernel (draw ids 7-9 at call `noise_step`, or the
// injected noise), the agent's training forward, the frozen prior's forward (forked onto aux_stream when given), the LOSS STAGE, net_backward
// into grad_theta -- with the loss stage passed in: it reads both networks' predictions and the targets, writes the three gradient seeds
// (and the per-crystal Lb / KLb scratch of the tape), enqueues on `s` only.  mi_ft_micro_step's stage is in backward.hip, mi_dpo_micro_step's in dpo.hip.
struct FtStageIO {
    const float *pl, *px, *pt, *plp, *pxp, *ptp;   // agent / prior predictions [B][9], [N][3], [N][100]
    const float *rl, *tx, *rt;                     // targets
    const int* node_off;                           // [B + 1]
    float *dl, *dx, *dt;                           // the seeds of the network backward, to be written for every row
    float *Lb, *KLb;                               // [B] each (the tape's)
    int B, N;
    float cl, cx, ct;
    int accum_steps;
};
typedef int (*ft_loss_stage_fn)(const FtStageIO& io, void* ctx, hipStream_t s);
int ft_micro_run(const char* what, mi_net* agent, mi_batch* ab, mi_net* prior, mi_batch* pb, const float* lengths, const float* angles,
                 const float* frac0, const int* atom_types, const float* time_freqs, int t, float c0, float c1, float sigma_t, float sigma_norm,
                 int copies, const int* ts, const float* c0s, const float* c1s, const float* sigmas, const float* sigma_norms, uint64_t seed,
                 uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t, float cost_lattice, float cost_coord,
                 float cost_type, int accum_steps, float* grad_theta, ft_loss_stage_fn stage, void* stage_ctx, void* stream, void* aux_stream);
int net_wgrad_window(mi_net* net, mi_batch* b, int slots);                   // 0: every backward contracts its own rows (default)
int net_wgrad_flush(mi_net* net, mi_batch* b, float* grad, hipStream_t s);   // grad += the pending micro-steps' node-level weight gradients
template <typename T>
int dev_alloc(mi_batch* b, T** p, size_t n);   // hipMalloc, or (pooled handle) a block of the pool: int / unsigned zero-filled, see pool.hip
void dev_release(mi_batch* b, void* p);        // one buffer of the handle, ahead of its destruction: hipFree, or back to the pool
// pool.hip: what a pooled handle asks of its pool.  kind = element type of the block: the typed hand-out of include/matinvent_hip_pool.h
enum PoolKind { POOL_INT = 0, POOL_F32 = 1, POOL_F16 = 2 };
hipStream_t pool_stream(const mi_pool* pool);
int pool_alloc(mi_pool* pool, size_t bytes, int kind, void** out);
void pool_release(mi_pool* pool, void* p);
void pool_handle_count(mi_pool* pool, int delta);
int pool_build_tables(mi_batch* b, hipStream_t s);   // the index tables of a pooled handle from node_off / edge_off / pair_off (device)
// a buffer's clear at set-up: the blocking hipMemset of a handle that owns its memory, or enqueued on the pool's stream
inline hipError_t batch_memset(const mi_batch* b, void* p, int v, size_t bytes) {
    return b->pool ? hipMemsetAsync(p, v, bytes, pool_stream(b->pool)) : hipMemset(p, v, bytes);
}
// the one-line checks of the entries: a pooled handle where none is taken; a pooled handle used on another stream than its pool's
#define MI_NO_POOLED(b, what) \
    MI_CHECK(!(b) || !(b)->pool, MI_EINVAL, "%s: a pooled batch handle is not taken here (include/matinvent_hip_pool.h lists the entries that take one)", what)
#define MI_NO_LATENT(net, what) \
    MI_CHECK(!(net) || (net)->Z == 0, MI_EINVAL, what ": the network has a property-conditioned embedding (mi_net_set_latent), which this entry does not fill (include/matinvent_hip_guidance.h lists the entries that do)")
#define MI_POOL_STREAM(b, stream, what) \
    MI_CHECK(!(b) || !(b)->pool || mi::pool_stream((b)->pool) == (hipStream_t)(stream), MI_EINVAL, what ": a pooled batch handle is used on its pool's stream only")
// input_grad.hip: the host-side refusals of the input-gradient path that need no launch, under the caller's name (MI_EINVAL / MI_ESTATE with the
// message set; net and b are not NULL): for an entry that enqueues work of its own in front of mi_scalar_input_grad (vib.hip, elastic.hip)
int input_grad_refusals(const char* what, const mi_net* net, const mi_batch* b);
// vib.hip, elastic.hip: the host-side check of a chunk's argument block over the fields mi_vib_chunk_args and mi_elastic_chunk_args share;
// family names the unit in the pooled-handle refusal, own_pointers is the unit's own non-null condition (read only where pointers are)
template <class Args>
int energy_chunk_check(const char* what, const char* family, const mi_batch* b, const Args* q, bool own_pointers) {
    MI_CHECK(b, MI_EINVAL, "%s: null handle", what);
    MI_CHECK(q, MI_EINVAL, "%s: null argument block", what);
    MI_NO_POOLED(b, family);
    MI_CHECK(pos_finite(q->h) && pos_finite(q->scale) && pos_finite(q->det_min), MI_EINVAL, "%s: h = %g, scale = %g, det_min = %g: each must be finite and positive",
             what, q->h, q->scale, q->det_min);
    MI_CHECK(q->Bs >= 0, MI_EINVAL, "%s: Bs = %d", what, q->Bs);
    if (b->B == 0 || b->N == 0) return MI_OK;
    MI_CHECK(q->src_types && q->src_frac && q->src_lat && q->src_node_off && q->plan_src && q->plan_copy && q->types && q->frac && q->lat && q->workspace &&
                 own_pointers,
             MI_EINVAL, "%s: null argument", what);
    MI_CHECK((((uintptr_t)q->types | (uintptr_t)q->src_types) & 15) == 0, MI_EINVAL, "%s: the type rows must be 16-byte aligned", what);
    return MI_OK;
}
// pretrain.hip: the supervised micro-step's sequence -- time gather, the EMBEDDING STAGE, noising, the network, loss, statistics, backward --
// with the embedding stage passed in: it fills b->temb [B][TD] from b->times on `s`.  mi_pretrain_micro_step's stage is the time embedding
// (pretrain.hip), mi_pretrain_micro_step_cond's the crystal embedding with condition dropout (guidance.hip).
typedef int (*pretrain_embed_stage_fn)(mi_net* net, mi_batch* b, const float* time_freqs, void* ctx, hipStream_t s);
int pretrain_micro_run(const char* what, mi_net* net, mi_batch* b, const float* lengths, const float* angles, const float* frac0, const int* atom_types,
                       const float* time_freqs, const int* t_host, const int* t_dev, const float* sched_table_dev, int T, uint64_t seed,
                       uint32_t noise_step, const float* rand_l, const float* rand_x, const float* rand_t, float cost_lattice, float cost_coord,
                       float cost_type, int b_global, int n_global, int accum_steps, float* grad_theta, float* stats, float* out_parts,
                       pretrain_embed_stage_fn stage, void* stage_ctx, void* stream);
// guidance.hip: the crystal embedding [time | property] into `out` (yhat == NULL: the null row for every crystal; `b`: the handle whose time
// map the time part reads, or NULL), mi_sampler_run's host-side check of a handle with guidance (MI_EINVAL with the message set), and
// p_c + gamma (p_c - p_u) over up to three arrays in one launch, in place in the p_c arrays
int crystal_embedding(const mi_net* net, const mi_batch* b, int B, const int* times, int t_all, const float* time_freqs, const float* prop_freqs,
                      const float* yhat, const int* have, const int* drop, float* out, hipStream_t s);
int guidance_check(const mi_net* net, const mi_batch* b, bool has_rec, const char* what);
int guidance_combine(float* pl, const float* ul, size_t nl, float* px, const float* ux, size_t nx, float* pt, const float* ut, size_t nt, float gamma,
                     hipStream_t s);
int knn_alloc(mi_batch* b, int max_neighbors, int cap_per_node);
// node_bwd.hip: the node-level BACKWARD chain between two edge stages of the backward pass as one launch per layer boundary
extern int g_node_bwd, g_node_bwd_min_blocks;
size_t node_bwd_pack_elems(int H);
bool node_bwd_supported(const mi_net* net, const mi_batch* b);
int node_bwd_pack(mi_net* net, int l, const float* W1, const float* Wn0, const float* Wn2, hipStream_t s);
int node_bwd(mi_net* net, mi_batch* b, int l, const float* dPQ, float* dh, float* dY, float* dXa, float* Xa, float* lnpart, unsigned* dcat_absmax, hipStream_t s);
// node_chain.hip: the node-level chain between two edge stages of an inference forward as one launch
bool node_chain_supported(const mi_net* net);
size_t node_chain_pack_elems(int H);
int node_chain_pack(mi_net* net, int l, const float* W1, const float* Wn0, const float* Wn2, const float* W2, hipStream_t s);
// edge_stage.hip: the second edge GEMM + edge -> node reduction on 128-row x H-column register tiles (inference, hidden_dim 512)
bool edge_gemm1_supported(const mi_net* net, int64_t M);
int edge_gemm1_pack(mi_net* net, int l, const float* W1, hipStream_t s);
bool edge_gemm2_supported(const mi_net* net);
extern int g_edge2_train;
extern int g_node_train;
extern int g_node_cols;
extern int g_ablate_skip;
int edge_gemm2(mi_net* net, mi_batch* b, int layer, hipStream_t s, float* Z2 = nullptr);   // Z2: optional pre-activation output (training forward)
int node_chain(mi_net* net, mi_batch* b, int l, hipStream_t s, bool train = false);
// stride.hip: the time embedding of a handle that carries a time map (steps: per-crystal step indices on the device, or NULL: k_all for every
// crystal), and the entries' host-side checks of the map (MI_EINVAL with the message set)
int time_embedding_mapped(const mi_batch* b, const int* steps, int k_all, const float* freqs, int B, int TD, float* out, hipStream_t s);
int time_map_check(const mi_batch* b, int T, const char* what);
int time_map_same(const mi_batch* p, const mi_batch* q, const char* what);
// condition.hip: mi_sampler_run's host-side check of the handle's condition (MI_EINVAL with the message set) and the imposition at `level`
// (one launch; rec_*: the record slices of that level, or NULL)
int condition_check(const mi_batch* b, int T, const char* what);
int condition_impose(const mi_batch* b, int level, uint64_t seed, float* atom_types, float* frac, float* lattices, float* rec_types, float* rec_frac,
                     float* rec_lat, hipStream_t s);
// sym_constraint.hip: mi_sampler_run's host-side check of a handle with a symmetry constraint (MI_EINVAL with the message set) and the
// projection of a state (one launch, none when every crystal has the identity alone)
int symmetry_check(const mi_batch* b, bool has_noise, bool has_rec, const char* what);
int symmetry_impose(const mi_batch* b, float* atom_types, float* frac, float* lattices, hipStream_t s);
// ... and the entries' host-side check that two handles of one call carry the same likelihood mask, or none (MI_EINVAL with the message set)
int likelihood_mask_same(const mi_batch* p, const mi_batch* q, const char* what);
// ... and the masked form of the sampler's predictor launch (logprob.h: PredictorArgs), for a recording chain on a handle with a condition and a mask
struct PredictorArgs;
int predictor_masked_launch(const mi_batch* b, const PredictorArgs& a, hipStream_t s);
// resample.hip: mi_sampler_run's host-side check of a handle with resampling (MI_EINVAL with the message set), the visited levels of a
// resampled chain (the one definition: mi_resample_schedule and the chain's driver read it), the per-visit seed and the forward jump
// from `from_level` to from_level + j (one launch)
int resample_check(const mi_batch* b, int T, int t_start, int t_stop, bool has_noise, bool has_rec, const char* what);
int resample_levels(int t_start, int r, int j, std::vector<int>* levels);
uint64_t resample_visit_seed(uint64_t seed, uint32_t v);
int resample_jump(const mi_batch* b, int from_level, uint64_t seed, float* atom_types, float* frac, float* lattices, hipStream_t s);
extern int g_knn_nosync;
int knn_build(mi_batch* b, const float* frac, const float* lattices, hipStream_t s, bool nosync = false);
}  // namespace mi
