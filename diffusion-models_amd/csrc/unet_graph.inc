// The shape of Unet.forward between init_conv and final_conv (DD/denoising_diffusion.py:349-390; text hooks
// DD/denoising_diffusion_text_conditional.py:131-214) as data: one node list that the inference walk (unet_forward_impl), the
// tape walk (unet_train_forward) and the backward walk (unet_train_backward_impl, in reverse) all run.  A value is a tensor
// of the walk; value 0 is init_conv's output (`r = x.clone()`, read again by final_res_block), -1 is none.

// Phase of the backward pass in which a parameter's stage is left (the order the reversed node list walks the network):
// 0 final_res_block / final_conv, 1 .. n the up stages (last first), n + 1 the middle, n + 2 .. 2n + 1 the down stages
// (last first), 2n + 2 what only the end of the pass completes (init_conv, the time / text MLPs)
static int grad_phase(const dm_unet* u, const std::string& name) {
    const int n = u->cfg.n_stages;
    auto starts = [&](const char* p) { return name.compare(0, std::strlen(p), p) == 0; };
    if (starts("final_res_block.") || starts("final_conv.")) return 0;
    if (starts("ups.")) return 1 + (n - 1 - std::atoi(name.c_str() + 4));
    if (starts("mid_") || starts("cross_attn")) return n + 1;
    if (starts("downs.")) return n + 2 + (n - 1 - std::atoi(name.c_str() + 6));
    return 2 * n + 2;
}

enum NodeKind { NODE_RESNET, NODE_ATTN, NODE_CROSS, NODE_CONV };  // NODE_CONV: the resample convolutions

struct UnetNode {
    NodeKind kind;
    const void* layer;  // the layer inside the handle: a ResBlock, AttnLayer, CrossLayer or ConvLayer, by kind
    const ResBlock& res() const { return *static_cast<const ResBlock*>(layer); }
    const AttnLayer& attn() const { return *static_cast<const AttnLayer*>(layer); }
    const CrossLayer& cross() const { return *static_cast<const CrossLayer*>(layer); }
    const ConvLayer& conv() const { return *static_cast<const ConvLayer*>(layer); }
    int in0, in1, out;  // value ids; in1: the skip connection of a ResnetBlock of the up path (x0 for final_res_block)
    int lin, lout;      // resolution level of input and output: h = H >> level
    int phase;          // grad_phase() of the layer's parameters
};

struct UnetGraph {
    std::vector<UnetNode> nodes;
    std::vector<int> last_use;  // per value: index of the node that reads it last (inference releases it there)
    int n_values() const { return (int)last_use.size(); }
    int out() const { return nodes.back().out; }  // final_res_block's output, what final_conv reads
};
enum { GRAPH_PLAIN, GRAPH_CROSS, GRAPH_CROSS1, N_GRAPHS };  // no CrossAttention layers / with them / the one-token shortcut

// cross: the three CrossAttention hooks around the bottleneck run.  dead: with one context token a CrossAttention ignores
// its image input (run_cross), so nothing between the last skip connection and cross_attn_up can reach the output: the
// list has no last down resample, cross_attn_down, mid_block1, cross_attn, mid_attn or mid_block2, and cross_attn_up has
// no image input.  The skip connections carry the image signal, exactly as in the reference.
static UnetGraph unet_graph(dm_unet* u, bool cross, bool dead) {
    UnetGraph g;
    g.last_use = {-1};  // value 0
    const int n = u->cfg.n_stages;
    auto node = [&](NodeKind kind, const void* layer, const std::string& param, int in0, int in1, int lin, int lout) {
        for (int v : {in0, in1})
            if (v >= 0) g.last_use[v] = (int)g.nodes.size();
        g.nodes.push_back(UnetNode{kind, layer, in0, in1, g.n_values(), lin, lout, grad_phase(u, param)});
        g.last_use.push_back(-1);
        return g.nodes.back().out;
    };
    auto resnet = [&](const ResBlock& R, int in0, int in1, int lv) { return node(NODE_RESNET, &R, R.prefix + ".", in0, in1, lv, lv); };
    auto attn = [&](const AttnLayer& A, int in, int lv) { return node(NODE_ATTN, &A, A.prefix + ".", in, -1, lv, lv); };
    auto crossn = [&](const CrossLayer& C, int in, int lv) { return node(NODE_CROSS, &C, C.prefix + ".", in, -1, lv, lv); };
    auto conv = [&](const ConvLayer& L, int in, int lin, int lout) { return node(NODE_CONV, &L, L.src.wname, in, -1, lin, lout); };
    std::vector<int> skips;
    int cur = 0, lv = 0;
    for (int i = 0; i < n; ++i) {
        const Stage& S = u->downs[i];
        const bool last = i == n - 1;
        cur = resnet(S.b1, cur, -1, lv);
        skips.push_back(cur);
        cur = resnet(S.b2, cur, -1, lv);
        cur = attn(S.attn, cur, lv);
        skips.push_back(cur);
        if (last && dead) continue;
        cur = conv(S.resample, cur, lv, last ? lv : lv + 1);
        lv = g.nodes.back().lout;
    }
    if (dead) {
        cur = crossn(u->cross_up, -1, lv);
    } else {  // each CrossAttention REPLACES x (:173-177, :187-191, :199-203)
        if (cross) cur = crossn(u->cross_down, cur, lv);
        cur = resnet(u->mid1, cur, -1, lv);
        if (cross) cur = crossn(u->cross_mid, cur, lv);
        cur = attn(u->mid_attn, cur, lv);
        cur = resnet(u->mid2, cur, -1, lv);
        if (cross) cur = crossn(u->cross_up, cur, lv);
    }
    for (int j = 0; j < n; ++j) {
        const Stage& S = u->ups[j];
        for (const ResBlock* R : {&S.b1, &S.b2}) {  // block1 takes attn's output of down stage n-1-j, block2 its block1's
            cur = resnet(*R, cur, skips.back(), lv);
            skips.pop_back();
        }
        cur = attn(S.attn, cur, lv);
        cur = conv(S.resample, cur, lv, j == n - 1 ? lv : lv - 1);
        lv = g.nodes.back().lout;
    }
    resnet(u->final_res, cur, 0, lv);
    return g;
}

// The three lists of a handle.  build_all has sized u->downs / u->ups before this point and a refresh re-packs the layers in
// place, so the pointers stay valid for the handle's life.
static void build_unet_graphs(dm_unet* u) {
    const bool has_cross = u->cfg.text_mode == DM_TEXT_CROSS;
    u->graphs = {unet_graph(u, false, false), has_cross ? unet_graph(u, true, false) : UnetGraph{},
                 has_cross ? unet_graph(u, true, true) : UnetGraph{}};  // GRAPH_PLAIN, GRAPH_CROSS, GRAPH_CROSS1
}
