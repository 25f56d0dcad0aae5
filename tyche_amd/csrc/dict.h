// dict.h -- what the host entry points (engine.hip: tyche_compress_host / tyche_decompress_host)
// need from the shared-dictionary layer (dict.hip): the process-wide dictionary a call runs with, the
// reach rule as one chunk launch, and the TYCHE_LZ4_DICT_AUTO hooks.
#pragma once
#include <mutex>

#include "engine.h"
#include "host_batch.h"

namespace tyche {

// What differs between the codecs (dict.hip): one constant for each of TYCHE_LZ4_COMPRESSOR_ID,
// TYCHE_ZSTD_COMPRESSOR_ID and TYCHE_ZLIB_COMPRESSOR_ID (the ids that may be asked for).
struct DictCodec;
const DictCodec &dict_codec(int compressor_id);

// The codec's process-wide dictionary for one host call, retained in get() and released with the
// hold; d stays NULL when none is installed.  get() is TYCHE_E_BAD_ARGS when the codec's environment
// variable names a dictionary that cannot serve.
struct DictHold {
    const tyche_lz4_dict_t *d = nullptr;
    int get(const DictCodec &c);
    ~DictHold();
};

// Why a dictionary upload inside a host-path launch failed.  The launch may run on a fan-out worker
// thread, whose error text the caller never sees, and run_host names only "kernel launch": the first
// reason is kept here and put back into the calling thread's text after the batch.
struct DictUploadNote {
    std::mutex mu;
    std::string msg;
    hipError_t upload(const tyche_lz4_dict_t *d, Lz4DictDev *img, const void **seed, int which);   // seed NULL: the image alone; which: DictCodec::seed
    int finish(int rc);
};

// The reach rule, as the launch of one run_host chunk.  The pages the dictionary reaches (length, or
// capacity when decoding, + dictionary <= 65536) take the dictionary kernel; a chunk that also holds
// larger ones runs `plain` first, for them, and the dictionary launch then redoes the pages in reach
// over whatever that left.
hipError_t dict_launch(const DictCodec &c, bool decode, const tyche_lz4_dict_t *d, DictUploadNote &note,
                       const tyche_batch_t &b, hipStream_t s, bool host_dst, LaunchRef plain);

// TYCHE_LZ4_DICT_AUTO: the sample, handed to the host compress call that completed it (dict_len != 0)
struct AutoSample {
    uint32_t dict_len = 0;
    std::vector<uint8_t> data;
    std::vector<uint32_t> len;
};
// An LZ4 host compress call after its dictionary lookup found d: LZ4_EXACT=1 refuses a dictionary,
// installed or still being collected for; without one, auto mode copies the call's eligible pages
// into the sample (never trains: that is auto_train_and_install, after the call's own pages).
int lz4_host_compress_rules(const tyche_lz4_dict_t *d, size_t n, const void *const *src, const uint32_t *src_lengths,
                            AutoSample *out);
// Trains on the completed sample and installs the result, unless something was installed (or auto
// mode ended: tyche_lz4_use_dict) meanwhile.  A failure leaves its reason in the thread's error
// text and the process plain.
void auto_train_and_install(const AutoSample &a);

}  // namespace tyche
