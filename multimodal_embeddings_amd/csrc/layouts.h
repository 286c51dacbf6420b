// The token layouts the library runs, one row each: what the host code between the kernels and the C ABI needs to know of
// a sequence layout (included by common.h, behind the geometry constants).  The launchers (kernels.h) and the *_apply
// hooks look a layout up here; the files that instantiate the kernels assert their instantiations against it, so a row
// that no kernel is built for does not compile.
#pragma once

enum AttnFamily {  // the file whose attention kernels run a layout
    ATTN_LONG,     // attention.hip: the guarded fast form and its exact re-run (launch_attention)
    ATTN_SHORT,    // attention_short.hip: attn_short<T, CAUSAL>, exact (launch_attention_exact)
    ATTN_MID       // attention_mid.hip: attn_mid, exact (launch_attention_exact)
};

struct TokenLayout {
    int tokens, patches;   // rows per sequence; patches per crop (0: a text layout)
    bool cls;              // row 0 of a crop is the class row
    int patch, patch_dim;  // image layouts: patch size and K of the patch-embed GEMM (3 patch^2, padded to 64); else 0
    bool embed_rows;       // image layouts: a row kernel writes the token rows behind an f32 patch-embed GEMM (197: EPI_PATCH does)
    bool causal;
    AttnFamily attn;
    int heads[3];          // the head counts (of 64) the attention is built for
    int blocks;            // query blocks of 32: only_block in -1 .. blocks - 1 (the causal layout takes -1 only)
    bool pooled;           // one row per sequence is pooled (image: pool_ln / pool_ln_l2; text: the EOS or last row)
    constexpr bool image() const { return patch != 0; }
    constexpr bool has_heads(int h) const { return h == heads[0] || h == heads[1] || h == heads[2]; }
    constexpr bool takes_block(int only_block) const { return only_block >= -1 && only_block < (causal ? 0 : blocks); }
};

constexpr TokenLayout LAYOUTS[] = {
    // tokens patches cls   patch dim  embed  causal family      heads        blocks pooled
    {197,    196,    true,  16, 768,  false, false, ATTN_LONG,  {6, 12, 16}, 7,     true},   // ViT/16, CLIP/16
    {196,    196,    false, 16, 768,  true,  false, ATTN_LONG,  {6, 12, 16}, 7,     false},  // SigLIP (pooling head)
    {50,     49,     true,  32, 3072, true,  false, ATTN_SHORT, {6, 12, 16}, 2,     true},   // ViT/32, CLIP/32
    {257,    256,    true,  14, 640,  true,  false, ATTN_MID,   {6, 12, 16}, 9,     true},   // DINOv2
    {77,     0,      false, 0,  0,    false, true,  ATTN_SHORT, {8, 12, 16}, 3,     true},   // CLIP text
    {64,     0,      false, 0,  0,    false, false, ATTN_SHORT, {8, 12, 16}, 2,     true},   // SigLIP text
};

// the row of a token count (no two rows share one), or null; with `causal`, only a row under that mask
constexpr const TokenLayout* find_layout(int tokens) {
    for (const TokenLayout& L : LAYOUTS)
        if (L.tokens == tokens) return &L;
    return nullptr;
}
constexpr const TokenLayout* find_layout(int tokens, bool causal) {
    const TokenLayout* L = find_layout(tokens);
    return L && L->causal == causal ? L : nullptr;
}

// For the static_asserts beside the instantiations: a file asserts that the rows it serves are as many as the layouts it
// instantiates kernels for, and that each of those is such a row; a row added here without its kernel fails there.
template <class Pred> constexpr int count_layouts(Pred pred) {
    int n = 0;
    for (const TokenLayout& L : LAYOUTS) n += pred(L) ? 1 : 0;
    return n;
}
constexpr int count_attn(AttnFamily f) { return count_layouts([f](const TokenLayout& L) { return L.attn == f; }); }
constexpr bool attn_row(AttnFamily f, int T, bool causal = false) { return find_layout(T, causal) && find_layout(T, causal)->attn == f; }

// every row against the arithmetic of an image cut into patches and a sequence cut into query blocks
constexpr bool layout_consistent(const TokenLayout& L) {
    const int grid = L.image() ? VIT_IMG / L.patch : 0;
    return find_layout(L.tokens) == &L && L.blocks == (L.tokens + 31) / 32 && (!L.image() || (L.patches == grid * grid && L.tokens == L.patches + (L.cls ? 1 : 0) && L.patch_dim == ((3 * L.patch * L.patch + 63) & ~63)));
}
static_assert(count_layouts(layout_consistent) == sizeof(LAYOUTS) / sizeof(LAYOUTS[0]), "layouts.h: a row shares its token count or contradicts its own patch size, class row or block count");
