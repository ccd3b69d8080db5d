// regen_ord.hpp — what names the action of an instance ordinal of VSR.tla (the numbering of gen<>, vsr_actions.hpp).  The claim bitmap of the deep search
// keeps one bit per (parent, ordinal); the kernel that regenerates a level from it (vsr_regen_bits.hpp) has no guard evaluation that would tell it which
// action a set bit belongs to, and finds it from the ordinal alone:
//   ordinals 0 .. m0-1 are bound to a replica and named by their range — TimerSendSVC(r), SendDVC(r), SendSV(r), ExecuteOp(r), R each, then
//   ReceiveClientRequest(r, c, v), R x C x |Values|;
//   ordinals m0 + j (R + 1) + k2 are bound to bag entry j: k2 = 0 is the receive action the entry's own guard names, k2 = d > 0 is SendGetState to replica d.
// Plain C++ with nothing of HIP and nothing of the record format in it: the kernel includes it with REGEN_ORD_FN set to its own function qualifiers, and
// tests/test_regen_ord.py builds it alone against the enumeration order of the oracle (tests/regen_ord_main.cpp).
#pragma once

#ifndef REGEN_ORD_FN
#define REGEN_ORD_FN inline
#endif

enum { REGEN_ORD_TIMER_SEND_SVC = 0, REGEN_ORD_SEND_DVC = 1, REGEN_ORD_SEND_SV = 2, REGEN_ORD_EXECUTE_OP = 3, REGEN_ORD_CLIENT_REQUEST = 4, REGEN_ORD_MESSAGE = 5 };

struct RegenOrd {
  int cls;        // REGEN_ORD_*: the first five name the action; REGEN_ORD_MESSAGE: the bag entry's guard does
  int r;          // replica-bound: the replica, 1-based
  int b;          // ReceiveClientRequest: the (client, value) pair, c * |Values| + v, 0-based
  int j, k2;      // message-bound: the bag entry; 0 = its receive action, d > 0 = SendGetState to replica d
};

REGEN_ORD_FN int regen_ord_m0(int R, int C, int n) { return 4 * R + R * C * n; }

REGEN_ORD_FN RegenOrd regen_ord(int R, int C, int n, int ord) {
  RegenOrd o = {REGEN_ORD_MESSAGE, 0, 0, 0, 0};
  const int m0 = regen_ord_m0(R, C, n);
  if (ord < 4 * R) {
    o.cls = ord / R;
    o.r = ord % R + 1;
  } else if (ord < m0) {
    o.cls = REGEN_ORD_CLIENT_REQUEST;
    o.r = (ord - 4 * R) / (C * n) + 1;
    o.b = (ord - 4 * R) % (C * n);
  } else {
    o.j = (ord - m0) / (R + 1);
    o.k2 = (ord - m0) % (R + 1);
  }
  return o;
}
