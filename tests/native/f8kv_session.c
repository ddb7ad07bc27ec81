/* f8kv_session.c -- SPT_MODEL_CROSS_KV_F8 as a C program sees it (tests/test_gpu_f8kv.py builds it -Wall
 * -Werror): the refusal of the f32 engine, then create -> info -> transcribe -> aligned refusal -> destroy.
 * Usage: f8kv_session <model spec> [--link-only] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spittle_hip.h"

#if !defined(SPT_HAS_CROSS_KV_F8) || SPT_MODEL_CROSS_KV_F8 != 4u
#error "the header does not announce the fp8 cross K/V cache"
#endif

#define CHECK(cond, what)                                       \
    do {                                                        \
        if (!(cond)) {                                          \
            fprintf(stderr, "f8kv_session: %s\n", what);        \
            return 1;                                           \
        }                                                       \
    } while (0)

int main(int argc, char** argv) {
    CHECK(argc >= 2, "usage: f8kv_session <model spec> [--link-only]");
    char err[256] = "";
    spt_model_params mp;
    spt_default_model_params(&mp);
    mp.max_batch = 2;
    /* refused before any device is looked for */
    mp.dtype = SPT_DTYPE_F32;
    mp.flags = SPT_MODEL_CROSS_KV_F8;
    spt_ctx* ctx = NULL;
    CHECK(spt_ctx_create(argv[1], &mp, &ctx, err, sizeof err) == SPT_ERR_UNSUPPORTED && !ctx, "the f32 engine took the flag");
    CHECK(spt_get_cross_kv_info(NULL, NULL, NULL, NULL) == SPT_ERR_INVALID_ARG, "info of a null context");
    if (argc > 2 && !strcmp(argv[2], "--link-only")) {
        printf("f8kv_session linked: %s\n", spt_version());
        return 0;
    }
    int64_t bytes16 = 0;
    for (int on = 0; on < 2; ++on) {
        mp.dtype = SPT_DTYPE_BF16;
        mp.flags = on ? SPT_MODEL_CROSS_KV_F8 : 0u;
        CHECK(spt_ctx_create(argv[1], &mp, &ctx, err, sizeof err) == SPT_OK, err);
        int32_t format = -1;
        int64_t cache = 0, staging = -1;
        CHECK(spt_get_cross_kv_info(ctx, &format, &cache, &staging) == SPT_OK, "cross_kv_info");
        spt_model_info info;
        CHECK(spt_ctx_info(ctx, &info) == SPT_OK, "ctx_info");
        if (!on) {
            CHECK(format == 0 && staging == 0 && cache > 0, "the unflagged context's cache");
            bytes16 = cache;
        } else {
            CHECK(format == 1 && staging > 0, "the flagged context's format");
            CHECK((double)cache <= 0.54 * (double)bytes16, "the fp8 cache is above 0.54 of the 16-bit one");
            CHECK(info.workspace_bytes > cache + staging, "workspace_bytes");
        }
        const size_t n = 16000 * 3;
        float* pcm = (float*)calloc(n, sizeof(float));
        CHECK(pcm, "calloc");
        for (size_t i = 0; i < n; ++i) pcm[i] = 0.1f * (float)((i * 2654435761u >> 16) & 0xFF) / 255.0f - 0.05f;
        spt_infer_params ip;
        spt_default_infer_params(&ip);
        ip.language = "en";
        ip.flags = SPT_NO_TIMESTAMPS | SPT_IGNORE_EOT | SPT_SUPPRESS_BLANK;
        ip.temperature_inc = 0.0f;
        ip.max_new_tokens = 6;
        spt_result* r = NULL;
        CHECK(spt_transcribe(ctx, pcm, n, &ip, &r) == SPT_OK && r, spt_last_error(ctx));
        CHECK(r->n_tokens == 6, "six tokens");
        spt_result_free(r);
        const size_t kv = (size_t)info.n_head * (size_t)info.n_audio_ctx * 64;
        float* k = (float*)malloc(kv * sizeof(float));
        float* v = (float*)malloc(kv * sizeof(float));
        CHECK(k && v, "malloc");
        CHECK(spt_debug_cross_kv(ctx, 0, 0, k, v) == SPT_OK, spt_last_error(ctx));
        CHECK(spt_debug_cross_kv(ctx, info.n_dec, 0, k, v) == SPT_ERR_INVALID_ARG, "a layer out of range");
        CHECK(spt_debug_cross_kv(ctx, 0, 1, k, v) == SPT_ERR_INVALID_ARG, "a window out of range");
        if (on) {
            spt_alignment* al = NULL;
            r = NULL;
            CHECK(spt_transcribe_aligned(ctx, pcm, n, &ip, &r, &al) == SPT_ERR_UNSUPPORTED && !r && !al, "aligned call");
            CHECK(strstr(spt_last_error(ctx), "CROSS_KV_F8") != NULL, "the refusal's message");
        }
        free(k);
        free(v);
        free(pcm);
        spt_ctx_destroy(ctx);
        ctx = NULL;
    }
    printf("f8kv_session ok\n");
    return 0;
}
