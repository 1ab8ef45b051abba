// coral_kmer_gpu.h - what coral_kmer.cpp (the C ABI of the k-mer counter) calls in coral_kmer.hip (the device backend).  Every
// function returns a CORAL_* code and leaves the reason in `err`.
#ifndef CORAL_KMER_GPU_H
#define CORAL_KMER_GPU_H

#include <stdint.h>

#include <map>
#include <string>

#include "coral_kmer_host.h"

namespace coral_kmer_gpu {

struct Device;                       // a device session: its streams, events, pinned staging buffers and the carved workspace

int64_t workspace_bytes(int k, int64_t staging_bytes);
void geometry(int32_t *out);
int open(int k, bool canonical, int device, uint32_t *table, int64_t staging_bytes, void *workspace, int64_t workspace_bytes, void *stream, uint64_t bases_before,
         Device **out, std::string &err);
int feed(Device *d, const uint8_t *bytes, int64_t n, std::string &err);
// waits for the stream; the statistics, the histogram and seconds[0..3] = upload, classify + compact, count, statistics
int finish(Device *d, coral_kmer::Stats &st, std::map<uint64_t, uint64_t> &hist, double *seconds, std::string &err);
int select(Device *d, uint64_t greater_than, int64_t capacity, uint64_t *kmers, uint32_t *counts, int64_t *n, std::string &err);      // device arrays
int lookup(Device *d, const uint64_t *indices, int64_t n, uint32_t *counts, std::string &err);                                          // device arrays
void close(Device *d);

}  // namespace coral_kmer_gpu
#endif /* CORAL_KMER_GPU_H */
