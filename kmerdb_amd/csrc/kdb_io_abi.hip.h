// kdb_io_abi.hip.h -- the entry points of include/kdbhip.h that take no engine and no device: the FASTA / FASTQ parsers, the BGZF and gzip
// readers, the .kdb row writer and reader (kdb_hostparse.cpp.h, kdb_kdbwriter.cpp.h).  Each checks its pointers, calls the host code and turns
// its reason into the thread's error message.
#pragma once
#include "kdb_hostutil.hip.h"
#include "kdb_hostparse.cpp.h"
#include "kdb_kdbwriter.cpp.h"

extern "C" {

int kdb_parse_fastq(const uint8_t *text, size_t n, int at_eof, uint8_t *bases_out, size_t bases_cap, uint64_t *offsets_out,
                    size_t cap_reads, uint64_t *header_spans_out, size_t *nreads_out, size_t *nbases_out, size_t *consumed_out)
{
    if ((!text && n) || !bases_out || !offsets_out || !nreads_out || !nbases_out || !consumed_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    int rc = kdbhost::parse_fastq(text, n, at_eof, bases_out, bases_cap, offsets_out, cap_reads, header_spans_out, nreads_out,
                                  nbases_out, consumed_out, &why);
    if (rc) return fail(KDB_ERR_ARG, "kdb_parse_fastq: %s", why);
    return KDB_OK;
}

int kdb_parse_fastq_mt(const uint8_t *text, size_t n, int at_eof, uint8_t *bases_out, size_t bases_cap, uint64_t *offsets_out,
                       size_t cap_reads, uint64_t *header_spans_out, size_t *nreads_out, size_t *nbases_out, size_t *consumed_out, int nthreads)
{
    if ((!text && n) || !bases_out || !offsets_out || !nreads_out || !nbases_out || !consumed_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    int rc = kdbhost::parse_fastq_mt(text, n, at_eof, bases_out, bases_cap, offsets_out, cap_reads, header_spans_out, nreads_out,
                                     nbases_out, consumed_out, &why, nthreads);
    if (rc) return fail(KDB_ERR_ARG, "kdb_parse_fastq: %s", why);
    return KDB_OK;
}

int kdb_parse_fasta(const uint8_t *text, size_t n, uint8_t *bases_out, size_t bases_cap, uint64_t *offsets_out, size_t cap_reads,
                    uint64_t *header_spans_out, size_t *nreads_out, size_t *nbases_out)
{
    if ((!text && n) || !bases_out || !offsets_out || !nreads_out || !nbases_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    int rc = kdbhost::parse_fasta(text, n, bases_out, bases_cap, offsets_out, cap_reads, header_spans_out, nreads_out, nbases_out, &why);
    if (rc) return fail(KDB_ERR_ARG, "kdb_parse_fasta: %s", why);
    return KDB_OK;
}

int kdb_parse_fasta_chunk(const uint8_t *text, size_t n, int at_eof, int in_record, uint8_t *bases_out, size_t bases_cap, uint64_t *offsets_out,
                          size_t cap_reads, uint64_t *header_spans_out, size_t *nreads_out, size_t *nbases_out, size_t *consumed_out, int *in_record_out)
{
    if ((!text && n) || !bases_out || !offsets_out || !nreads_out || !nbases_out || !consumed_out || !in_record_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    int rc = kdbhost::parse_fasta_chunk(text, n, at_eof, in_record, bases_out, bases_cap, offsets_out, cap_reads, header_spans_out, nreads_out, nbases_out,
                                        consumed_out, in_record_out, &why);
    if (rc) return fail(KDB_ERR_ARG, "kdb_parse_fasta_chunk: %s", why);
    return KDB_OK;
}

int kdb_bgzf_inflate(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, int nthreads, size_t *consumed_out, size_t *produced_out)
{
    if ((!src && n) || !dst || !consumed_out || !produced_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    if (kdbhost::bgzf_inflate(src, n, dst, cap, nthreads, consumed_out, produced_out, &why)) return fail(KDB_ERR_ARG, "kdb_bgzf_inflate: %s", why);
    return KDB_OK;
}

int kdb_bgzf_scan(const char *path, uint64_t *coff_out, uint64_t *uoff_out, size_t cap, size_t *n_out)
{
    if (!path || !coff_out || !uoff_out || !n_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    const int rc = kdbhost::bgzf_scan(path, coff_out, uoff_out, cap, n_out, &why);
    if (rc == 2) return fail(KDB_ERR_NOMEM, "kdb_bgzf_scan('%s'): %s", path, why);
    if (rc) return fail(KDB_ERR_ARG, "kdb_bgzf_scan('%s'): %s", path, why);
    return KDB_OK;
}

struct kdb_gz { kdbhost::GzStream *s; };

int kdb_gz_open(const char *path, kdb_gz **out)
{
    if (!path || !out) return fail(KDB_ERR_ARG, "NULL argument");
    *out = nullptr;
    const char *why = "";
    kdbhost::GzStream *s = kdbhost::gz_open(path, &why);
    if (!s) return fail(KDB_ERR_ARG, "kdb_gz_open('%s'): %s", path, why);
    *out = new kdb_gz{s};
    return KDB_OK;
}

int kdb_gz_read(kdb_gz *g, uint8_t *dst, size_t cap, size_t *n_out)
{
    if (!g || (!dst && cap) || !n_out) return fail(KDB_ERR_ARG, "NULL argument");
    *n_out = 0;
    if (g->s->read(dst, cap, n_out)) return fail(KDB_ERR_ARG, "kdb_gz_read: %s", g->s->err.c_str());
    return KDB_OK;
}

int kdb_gz_close(kdb_gz *g)
{
    if (!g) return KDB_OK;
    delete g->s;
    delete g;
    return KDB_OK;
}

int kdb_write_kdb_rows_ex(const char *path, const uint64_t *counts, uint64_t nbins, uint64_t total_kmers, int compresslevel,
                          int nthreads, int encoder, uint64_t *nblocks_out)
{
    if (!path || (!counts && nbins)) return fail(KDB_ERR_ARG, "NULL argument");
    if (encoder != KDB_ENCODER_DEFAULT && encoder != KDB_ENCODER_ROWS && encoder != KDB_ENCODER_ZLIB)
        return fail(KDB_ERR_ARG, "kdb_write_kdb_rows: unknown encoder %d", encoder);
    if (compresslevel < 0 || compresslevel > 9) return fail(KDB_ERR_ARG, "kdb_write_kdb_rows: compresslevel %d (0..9)", compresslevel);
    const char *why = "";
    if (kdbhost::write_kdb_rows(path, counts, nbins, total_kmers, compresslevel, nthreads, nblocks_out, &why, encoder))
        return fail(KDB_ERR_ARG, "kdb_write_kdb_rows('%s'): %s", path, why);
    return KDB_OK;
}

int kdb_write_kdb_rows(const char *path, const uint64_t *counts, uint64_t nbins, uint64_t total_kmers, int compresslevel,
                       int nthreads, uint64_t *nblocks_out)
{
    return kdb_write_kdb_rows_ex(path, counts, nbins, total_kmers, compresslevel, nthreads, KDB_ENCODER_DEFAULT, nblocks_out);
}

int kdb_read_kdb_rows(const char *path, uint64_t nbins, uint64_t *kmer_ids_out, uint64_t *counts_out, double *frequencies_out, int nthreads,
                      uint64_t *nrows_out)
{
    if (!path || !kmer_ids_out || !counts_out || !frequencies_out || !nrows_out) return fail(KDB_ERR_ARG, "NULL argument");
    const char *why = "";
    const int rc = kdbhost::read_kdb_rows(path, nbins, kmer_ids_out, counts_out, frequencies_out, nthreads, nrows_out, &why);
    if (rc == 3) return fail(KDB_ERR_STATE, "kdb_read_kdb_rows('%s'): not a file of BGZF members", path);
    if (rc) return fail(KDB_ERR_ARG, "kdb_read_kdb_rows('%s'): %s", path, why);
    return KDB_OK;
}

int kdb_format_frequency(uint64_t count, uint64_t total, char *buf, size_t cap)
{
    if (!buf || cap < 40) return fail(KDB_ERR_ARG, "buffer too small");
    int n = kdbhost::py_float_repr((double)count / (double)total, buf);
    buf[n] = 0;
    return KDB_OK;
}

}  // extern "C"
