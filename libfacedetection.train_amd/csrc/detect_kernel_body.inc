// detect_kernel_body.inc -- the body of detect.hip's kernels, included once per kernel template:
//   detect_kernel       SOFT = false: compaction, sort, decode, greedy NMS (`iou_thr`);
//   detect_soft_kernel  SOFT = true:  compaction, sort, decode, Soft-NMS rounds (`soft`).
// Text inclusion, not an inlined function (as loss_kernel_body.inc): wrapped in a function the greedy instances schedule
// differently, and they are to keep the code they had before Soft-NMS existed (profiles/soft_nms_codegen.txt).
// In scope: the kernel's arguments, `constexpr bool SOFT`, `iou_thr` and `soft` (YunetSoftNms; unread when !SOFT).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* skeys = reinterpret_cast<unsigned long long*>(smem);           // [lds_keys]
    float4* sbox = reinterpret_cast<float4*>(smem + (size_t)lds_keys * 8);             // [DET_BOX_CAP]
    __shared__ int s_k;
    const int n = blockIdx.x, tid = threadIdx.x;
    // FROM_HEAD: flat = [N,P,16] head outputs; else flat = [N,P,4] boxes with in_scores [N,P] and an
    // optional per-set element count (yunet_nms: the merged candidates of test-time augmentation)
    const FlatSrc hsrc{flat + (size_t)n * P * 16, L};
    const BoxSrc bsrc{flat + (size_t)n * P * 4, in_scores ? in_scores + (size_t)n * P : nullptr};
    const int Pn = (!FROM_HEAD && in_count) ? min(in_count[n], P) : P;
    unsigned char* sc = scratch + (size_t)n * ((size_t)P * 16 + (size_t)padP * 8);
    float4* gbox = reinterpret_cast<float4*>(sc);
    unsigned long long* gkeys = reinterpret_cast<unsigned long long*>(sc + (size_t)P * 16);
    const bool small = padP <= lds_keys;       // every prior fits in LDS: no global key traffic at all

    // ---- scores, threshold, compaction (order is irrelevant: the keys are sorted next) -----------------
    if (tid == 0) s_k = 0;
    __syncthreads();
    for (int p = tid; p < Pn; p += DET_THREADS) {
        float sc_;
        const bool ok = FROM_HEAD ? hsrc.score(p, score_thr, sc_) : bsrc.score(p, score_thr, sc_);
        if (ok) {
            const unsigned long long key =
                ((unsigned long long)score_key(sc_) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
            const int slot = atomicAdd(&s_k, 1);
            if (small) skeys[slot] = key;
            else gkeys[slot] = key;
        }
    }
    __syncthreads();
    const int K = s_k;
    int padn = 2;
    while (padn < K) padn <<= 1;
    float* dn = dets + (size_t)n * max_out * 5;
    float* kn = kps_out ? kps_out + (size_t)n * max_out * 10 : nullptr;
    int32_t* kp = keep ? keep + (size_t)n * max_out : nullptr;
    auto run = [&](auto keys) {
        if constexpr (FROM_HEAD) sort_decode_nms<SOFT>(keys, padn, K, hsrc, iou_thr, soft, max_out, gbox, sbox, dn, kn, kp, count + n);
        else sort_decode_nms<SOFT>(keys, padn, K, bsrc, iou_thr, soft, max_out, gbox, sbox, dn, kn, kp, count + n);
    };
    if (padn <= lds_keys) {
        if (!small)
            for (int i = tid; i < K; i += DET_THREADS) skeys[i] = gkeys[i];
        for (int i = K + tid; i < padn; i += DET_THREADS) skeys[i] = 0ull;
        __syncthreads();
        run(skeys);
    } else {
        for (int i = K + tid; i < padn; i += DET_THREADS) gkeys[i] = 0ull;
        __syncthreads();
        run(gkeys);
    }
