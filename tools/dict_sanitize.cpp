// dict_sanitize.cpp -- a stand-alone walk over the host side of the shared-dictionary layer
// (tyche_amd/csrc/dict.hip) for AddressSanitizer / UBSan.  It needs no GPU: every call here ends
// before a launch.  Build dict.hip, engine.hip and host_batch.hip with the sanitizers and link them,
// the library's other objects and this file into one program (not into Python):
//
//   S="-fsanitize=address,undefined"
//   hipcc --offload-arch=gfx950 -O1 -g -fPIC -std=c++17 -Iinclude -Xarch_host $S -c tyche_amd/csrc/dict.hip -o dict.o
//         (the same for engine.hip and host_batch.hip)
//   clang++ -O1 -g -std=c++17 -Iinclude $S -c tools/dict_sanitize.cpp -o main.o
//   hipcc --offload-arch=gfx950 -Xarch_host $S main.o dict.o engine.o host_batch.o \
//         <build/tyche_amd/*.o but those three, errno_guard.o last> -lpthread -o dict_sanitize
//   ./dict_sanitize          -> "dict_sanitize ok", exit 0, no sanitizer report
//
// What it does: create / retain (the slots, tyche_*_current_dict) / release; install, replace and
// remove in all three slots (LZ4, zstd, zlib) from two threads at once; tyche_lz4_dict_bytes; and, in a
// fresh child process each (the variables are read once per process), TYCHE_LZ4_DICT, TYCHE_ZSTD_DICT
// and TYCHE_ZLIB_DICT naming an empty, an over-long and a good file.
#include <spawn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <unistd.h>

#include <string>
#include <thread>
#include <vector>

#include "tyche_codec.h"

extern char **environ;

#define CHECK(c)                                                                       \
    do {                                                                               \
        if (!(c)) {                                                                    \
            fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, tyche_last_error()); \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

// the three slots: the codec of each, its variable, its install and its read call
struct Slot {
    int codec;
    const char *var;
    int (*use)(const tyche_dict_t *);
    tyche_dict_t *(*current)(void);
};
static const Slot kSlots[3] = {{TYCHE_LZ4_COMPRESSOR_ID, "TYCHE_LZ4_DICT", tyche_lz4_use_dict, tyche_lz4_current_dict},
                               {TYCHE_ZSTD_COMPRESSOR_ID, "TYCHE_ZSTD_DICT", tyche_zstd_use_dict, tyche_zstd_current_dict},
                               {TYCHE_ZLIB_COMPRESSOR_ID, "TYCHE_ZLIB_DICT", tyche_zlib_use_dict, tyche_zlib_current_dict}};

static int host_compress(int codec) {
    uint8_t page[100] = {0}, out[800];
    const void *src = page;
    void *dst = out;
    uint32_t slen = sizeof(page), dcap = sizeof(out);
    int32_t res = 0;
    return tyche_compress_host(codec, 1, 1, &src, &slen, &dst, &dcap, &res);
}

// child: the variable `var` (already in the environment) names a file; `want` is the error text it
// must give ("" for a file that serves, of `len` bytes)
static int env_child(const char *var, const char *want, uint32_t len) {
    const Slot *own = nullptr;
    for (const Slot &s : kSlots)
        if (strcmp(var, s.var) == 0) own = &s;
    CHECK(own);
    tyche_lz4_dict_t *cur = own->current();
    for (const Slot &s : kSlots)
        if (&s != own) CHECK(!s.current());   // the other slots read nothing
    const int rc = host_compress(own->codec);
    if (*want) {
        CHECK(!cur && rc == TYCHE_E_BAD_ARGS);
        CHECK(strstr(tyche_last_error(), var) && strstr(tyche_last_error(), want));
    } else {
        CHECK(cur && tyche_lz4_dict_length(cur) == len && rc != TYCHE_E_BAD_ARGS);
        tyche_lz4_dict_destroy(cur);
        CHECK(own->use(NULL) == TYCHE_E_OK);   // the slot's reference goes
    }
    for (const Slot &s : kSlots)
        if (&s != own) CHECK(host_compress(s.codec) != TYCHE_E_BAD_ARGS);
    return 0;
}

static void run_env_child(const char *var, const std::string &path, const char *want, uint32_t len) {
    std::vector<std::string> env;
    for (char **e = environ; *e; e++)
        if (strncmp(*e, "TYCHE_LZ4_DICT", 14) != 0 && strncmp(*e, "TYCHE_ZSTD_DICT", 15) != 0 &&
            strncmp(*e, "TYCHE_ZLIB_DICT", 15) != 0)
            env.push_back(*e);
    env.push_back(std::string(var) + "=" + path);
    std::vector<char *> envp;
    for (auto &e : env) envp.push_back(&e[0]);
    envp.push_back(nullptr);
    const std::string n = std::to_string(len);
    const char *argv[] = {"dict_sanitize", "env", var, want, n.c_str(), nullptr};
    pid_t pid = 0;
    int st = -1;
    CHECK(posix_spawn(&pid, "/proc/self/exe", nullptr, nullptr, (char *const *)argv, envp.data()) == 0);
    CHECK(waitpid(pid, &st, 0) == pid);
    if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) {
        fprintf(stderr, "child %s=%s failed (status %d)\n", var, path.c_str(), st);
        exit(1);
    }
}

static void write_file(const std::string &path, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    CHECK(f);
    std::vector<uint8_t> b(n, 0x5A);
    if (n) CHECK(fwrite(b.data(), 1, n, f) == n);
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc == 5 && strcmp(argv[1], "env") == 0) return env_child(argv[2], argv[3], (uint32_t)atol(argv[4]));

    // the environment files first, each in a child of a process that has made no device call yet
    char dir[] = "/tmp/dict_sanitize.XXXXXX";
    CHECK(mkdtemp(dir));
    const std::string empty = std::string(dir) + "/empty", big = std::string(dir) + "/big", good = std::string(dir) + "/good";
    write_file(empty, 0);
    write_file(big, TYCHE_LZ4_DICT_MAX + 1u);
    write_file(good, 4096);
    for (const char *var : {"TYCHE_LZ4_DICT", "TYCHE_ZSTD_DICT", "TYCHE_ZLIB_DICT"}) {
        run_env_child(var, empty, "is empty", 0);
        run_env_child(var, big, "longer than", 0);
        run_env_child(var, good, "", 4096);
    }
    for (const std::string &p : {empty, big, good}) unlink(p.c_str());
    rmdir(dir);

    // create / release, the refusals of create, and the bytes
    CHECK(!tyche_lz4_dict_create(NULL, 10) && !tyche_lz4_dict_create("x", 0));
    std::vector<uint8_t> blob(TYCHE_LZ4_DICT_MAX + 1u);
    for (size_t i = 0; i < blob.size(); i++) blob[i] = (uint8_t)(i * 131u >> 3);
    CHECK(!tyche_lz4_dict_create(blob.data(), (uint32_t)blob.size()));
    for (uint32_t len : {1u, 4u, 5u, 63u, 64u, 65u, 4097u, (uint32_t)TYCHE_LZ4_DICT_MAX}) {
        tyche_lz4_dict_t *d = tyche_lz4_dict_create(blob.data(), len);
        CHECK(d && tyche_lz4_dict_length(d) == len);
        std::vector<uint8_t> out(len + 8u, 0xEE);
        CHECK(tyche_lz4_dict_bytes(d, out.data(), len) == len && memcmp(out.data(), blob.data(), len) == 0 && out[len] == 0xEE);
        CHECK(tyche_lz4_dict_bytes(d, out.data(), 1) == len && tyche_lz4_dict_bytes(d, NULL, 0) == len);
        tyche_lz4_dict_destroy(d);
    }
    CHECK(tyche_lz4_dict_bytes(NULL, blob.data(), 4) == 0 && tyche_lz4_dict_length(NULL) == 0);
    tyche_lz4_dict_destroy(NULL);

    // two threads install, replace, read and remove in all three slots; each drops its creator's reference
    // while the slot may still hold the handle
    auto worker = [&](uint32_t seed) {
        for (uint32_t k = 0; k < 2000; k++) {
            const uint32_t len = 64u + (seed * 977u + k * 31u) % 2048u;
            tyche_lz4_dict_t *d = tyche_lz4_dict_create(blob.data() + (k & 255u), len);
            CHECK(d);
            CHECK(kSlots[(k + seed) % 3u].use(d) == TYCHE_E_OK);
            tyche_lz4_dict_destroy(d);
            for (tyche_lz4_dict_t *cur : {tyche_lz4_current_dict(), tyche_zstd_current_dict(), tyche_zlib_current_dict()})
                if (cur) {
                    uint8_t head[16];
                    CHECK(tyche_lz4_dict_bytes(cur, head, sizeof(head)) == tyche_lz4_dict_length(cur));
                    tyche_lz4_dict_destroy(cur);
                }
            if (k % 7u == 0) CHECK(kSlots[k % 3u].use(NULL) == TYCHE_E_OK);
            if (k % 97u == 0) (void)host_compress(kSlots[(k + seed) % 3u].codec);
        }
    };
    std::thread a(worker, 1u), b(worker, 2u);
    a.join();
    b.join();
    for (const Slot &s : kSlots) CHECK(s.use(NULL) == TYCHE_E_OK && !s.current());

    // a structured dictionary: zstd's slot refuses it, LZ4's and zlib's take it
    const uint8_t magic[8] = {0x37, 0xA4, 0x30, 0xEC, 1, 2, 3, 4};
    tyche_lz4_dict_t *m = tyche_lz4_dict_create(magic, sizeof(magic));
    CHECK(m && tyche_zstd_use_dict(m) == TYCHE_E_BAD_ARGS && tyche_lz4_use_dict(m) == TYCHE_E_OK);
    CHECK(tyche_zlib_use_dict(m) == TYCHE_E_OK && tyche_zlib_use_dict(NULL) == TYCHE_E_OK);
    CHECK(tyche_lz4_use_dict(NULL) == TYCHE_E_OK);
    tyche_lz4_dict_destroy(m);
    puts("dict_sanitize ok");
    return 0;
}
