// answers.cpp — the intake of the two optional inputs beside a batch's bindings (kp_host.h):
// their checks, with the texts every entry point reports, and the rows brought onto the
// device in rank order.
#include "kp_host.h"

namespace kp::host {

static int bad_answers(kp_engine* e, const char* who, const std::string& why) {
  e->err = std::string(who) + ": " + why;
  return KP_EINVAL;
}
static int check_clusters(kp_engine* e, const kp_snapshot* s, const char* who, const char* pre, uint64_t n_clusters) {
  if (n_clusters == (uint64_t)s->C) return KP_OK;
  return bad_answers(e, who, std::string(pre) + "n_clusters is " + std::to_string(n_clusters) +
                                 ", the snapshot holds " + std::to_string(s->C) + " clusters");
}
static int check_n_rows(kp_engine* e, const char* who, const char* pre, uint32_t n_rows) {
  if (n_rows <= (uint32_t)INT32_MAX) return KP_OK;
  std::string p(pre);  // ("est->" names the input here as "est: ")
  if (!p.empty()) p.replace(p.size() - 2, 2, ": ");
  return bad_answers(e, who, p + "more than 2^31 - 1 rows");
}

int check_row_of(kp_engine* e, const char* who, const char* pre, const int32_t* row_of, uint64_t first, uint64_t count,
                 uint32_t n_rows) {
  for (uint64_t k = first; k < first + count; k++)
    if (row_of[k] < -1 || row_of[k] >= (int64_t)n_rows)
      return bad_answers(e, who, std::string(pre) + "row_of[" + std::to_string(k) + "] = " + std::to_string(row_of[k]) +
                                     " is outside -1.." + std::to_string((int64_t)n_rows - 1));
  return KP_OK;
}

int check_estimates(kp_engine* e, const kp_snapshot* s, const char* who, const char* pre, const kp_estimates* est,
                    uint64_t n) {
  if (!est || est->n_rows == 0) return KP_OK;
  const std::string p(pre);
  if (int rc = check_clusters(e, s, who, pre, est->n_clusters)) return rc;
  if (!est->rows || (n && !est->row_of)) return bad_answers(e, who, p + "rows or " + p + "row_of is null");
  if (int rc = check_n_rows(e, who, pre, est->n_rows)) return rc;
  if (int rc = check_row_of(e, who, pre, est->row_of, 0, n, est->n_rows)) return rc;
  const size_t cells = (size_t)est->n_rows * s->C;
  for (size_t k = 0; k < cells; k++)  // (the first one in caller order)
    if (est->rows[k] < -1)
      return bad_answers(e, who, p + "rows[" + std::to_string(k / s->C) + "][" + std::to_string(k % s->C) + "] = " +
                                     std::to_string(est->rows[k]) + " is below -1 (UnauthenticReplica)");
  return KP_OK;
}

int check_filters(kp_engine* e, const kp_snapshot* s, const char* who, const char* pre, const kp_filter_answers* flt,
                  uint64_t n) {
  if (!flt || flt->n_rows == 0) return KP_OK;
  const std::string p(pre);
  if (int rc = check_clusters(e, s, who, pre, flt->n_clusters)) return rc;
  if (!flt->rows) return bad_answers(e, who, p + "rows is null");
  if (n && !flt->row_of) return bad_answers(e, who, p + "row_of is null");
  if (flt->n_plugins == 0)
    return bad_answers(e, who, p + "n_rows is " + std::to_string(flt->n_rows) + " with n_plugins == 0");
  return check_n_rows(e, who, pre, flt->n_rows);
}

// dev row bit rank = caller row bit perm[rank]; caller bits at or above C are never read.
int make_answer_rows(kp_engine* e, const kp_snapshot* s, const kp_estimates* est, const kp_filter_answers* flt,
                     dev::stream_t st, Arena* staging, const dev::event_t* tev,
                     std::shared_ptr<const AnswerRows>* out) {
  auto r = std::make_shared<AnswerRows>();
  int32_t* d_est_src = nullptr;
  uint64_t* d_flt_src = nullptr;
  r->dev.pool_dev = staging->pool_dev = e->device;
  if (est) {
    r->n_est = est->n_rows;
    staging->add(&d_est_src, est->rows, (size_t)est->n_rows * s->C);
    r->dev.add(&r->d_est, (size_t)est->n_rows * s->Cp);
  }
  if (flt) {
    r->n_flt = flt->n_rows;
    staging->add(&d_flt_src, flt->rows, (size_t)flt->n_rows * (((size_t)s->C + 63) / 64));
    r->dev.add(&r->d_flt, (size_t)flt->n_rows * s->W);
  }
  HIPCHK(r->dev.alloc());
  *out = r;  // (before anything is queued: the caller holds what the queued work writes)
  HIPCHK(staging->alloc());
  HIPCHK(staging->upload(st));
  if (tev) HIPCHK(dev::event_record(tev[0], st));
  if (est) HIPCHK(dev::est_rows_rank(st, s->view, d_est_src, (int)est->n_rows, r->d_est));
  if (tev) HIPCHK(dev::event_record(tev[1], st));
  if (flt) HIPCHK(dev::flt_rows_rank(st, s->view, d_flt_src, (int)flt->n_rows, r->d_flt));
  if (tev) HIPCHK(dev::event_record(tev[2], st));
  return KP_OK;
}

}  // namespace kp::host
