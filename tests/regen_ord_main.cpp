// Stand-alone check of csrc/regen_ord.hpp (tests/test_regen_ord.py builds and runs it, with sanitizers): every instance ordinal of VSR.tla goes through
// regen_ord() and the result is held against the order in which the oracle's `successors` enumerates the same instances (oracle/vsr_oracle.cpp: the actions
// in the order of Next, inside an action the replica ascending, then the client, then the value) — for R = 3 with one and with two clients, one to three
// values, and for R = 2.
#include <algorithm>
#include <cstdio>
#include <tuple>
#include <vector>

#include "regen_ord.hpp"

namespace {
// the action ids of the oracle (oracle/vsr_oracle.hpp) and of the library (csrc/vsr_model.hpp): the position in Next
enum { A_TimerSendSVC = 1, A_SendDVC = 4, A_SendSV = 7, A_ReceiveClientRequest = 9, A_ExecuteOp = 12 };

int action_of(int cls) {
  switch (cls) {
    case REGEN_ORD_TIMER_SEND_SVC: return A_TimerSendSVC;
    case REGEN_ORD_SEND_DVC: return A_SendDVC;
    case REGEN_ORD_SEND_SV: return A_SendSV;
    case REGEN_ORD_EXECUTE_OP: return A_ExecuteOp;
    case REGEN_ORD_CLIENT_REQUEST: return A_ReceiveClientRequest;
  }
  return -1;
}

typedef std::tuple<int, int, int, int> Inst;   // action, replica, client, value

int check(int R, int C, int n) {
  // the oracle's order over the replica-bound instances
  std::vector<Inst> want;
  for (int a : {A_TimerSendSVC, A_SendDVC, A_SendSV}) for (int r = 1; r <= R; r++) want.push_back(Inst(a, r, 0, 0));
  for (int r = 1; r <= R; r++) for (int c = 1; c <= C; c++) for (int v = 1; v <= n; v++) want.push_back(Inst(A_ReceiveClientRequest, r, c, v));
  for (int r = 1; r <= R; r++) want.push_back(Inst(A_ExecuteOp, r, 0, 0));
  const int m0 = regen_ord_m0(R, C, n);
  if (m0 != (int)want.size()) { std::printf("m0 %d != %zu\n", m0, want.size()); return 1; }
  std::vector<std::pair<Inst, int>> got;       // (instance, ordinal)
  for (int ord = 0; ord < m0; ord++) {
    const RegenOrd o = regen_ord(R, C, n, ord);
    if (o.cls == REGEN_ORD_MESSAGE || o.r < 1 || o.r > R) { std::printf("ordinal %d: class %d replica %d\n", ord, o.cls, o.r); return 1; }
    if (o.cls == REGEN_ORD_CLIENT_REQUEST) {
      if (o.b < 0 || o.b >= C * n) { std::printf("ordinal %d: pair %d\n", ord, o.b); return 1; }
      got.push_back({Inst(action_of(o.cls), o.r, o.b / n + 1, o.b % n + 1), ord});
    } else {
      got.push_back({Inst(action_of(o.cls), o.r, 0, 0), ord});
    }
  }
  // by action in the order of Next, the ordinals of one action ascending: the oracle's enumeration, instance for instance
  std::stable_sort(got.begin(), got.end(), [](const std::pair<Inst, int>& x, const std::pair<Inst, int>& y) { return std::get<0>(x.first) < std::get<0>(y.first); });
  for (size_t i = 0; i < want.size(); i++)
    if (got[i].first != want[i]) { std::printf("R %d C %d n %d: instance %zu differs (ordinal %d)\n", R, C, n, i, got[i].second); return 1; }
  // the message-bound ordinals: bag entry j ascending, inside it k2 = 0 (the entry's receive action) then SendGetState to replica 1 .. R; every pair once
  int ord = m0;
  for (int j = 0; j < 64; j++)
    for (int k2 = 0; k2 <= R; k2++, ord++) {
      const RegenOrd o = regen_ord(R, C, n, ord);
      if (o.cls != REGEN_ORD_MESSAGE || o.j != j || o.k2 != k2) { std::printf("R %d C %d n %d: ordinal %d -> class %d entry %d k2 %d\n", R, C, n, ord, o.cls, o.j, o.k2); return 1; }
    }
  return 0;
}
}  // namespace

int main() {
  int checked = 0;
  for (int R = 2; R <= 3; R++)
    for (int C = 1; C <= 2; C++)
      for (int n = 1; n <= 3; n++) {
        if (check(R, C, n)) return 1;
        checked++;
      }
  std::printf("ok %d\n", checked);
  return 0;
}
