"""CPU stand-ins for the device side of the backward pass, for tests/test_tacotron_backward_cpu.py: the recurrences of
csrc/facppg_taco_bwd.hip step by step in torch (``EmuRec``, the interface of common.taco_grad.HipRecurrences), and the
teacher-forced forward pass in torch (``torch_forward``) for the states the backward pass reads.  With them
``common.taco_grad.backward`` runs on the CPU in float64, where it can be held to the float64 reference directly."""
import torch
import torch.nn.functional as F

from common import taco_grad as tg


class EmuRec:
    def cell_scan(self, pre, lengths=None):
        pre = pre.detach()
        N, T, H4 = pre.shape; H = H4 // 4
        act = torch.zeros_like(pre); c = torch.zeros(N, T, H)
        cs = torch.zeros(N, H)
        for t in range(T):
            v = torch.ones(N, 1, dtype=torch.bool) if lengths is None else (t < lengths.long())[:, None]
            g = pre[:, t]
            a = torch.cat([torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2*H]), torch.tanh(g[:, 2*H:3*H]), torch.sigmoid(g[:, 3*H:])], 1)
            cn = a[:, H:2*H] * cs + a[:, :H] * a[:, 2*H:3*H]
            cs = torch.where(v, cn, cs)
            act[:, t] = torch.where(v, a, torch.zeros_like(a)); c[:, t] = torch.where(v, cn, torch.zeros_like(cn))
        return act, c

    @staticmethod
    def cell_bwd(act, c, t, dh, dcn):
        H = c.shape[2]
        a = act[:, t]; gi, gf, gg, go = a[:, :H], a[:, H:2*H], a[:, 2*H:3*H], a[:, 3*H:]
        ct = c[:, t]; cp = c[:, t-1] if t > 0 else torch.zeros_like(ct)
        tc = torch.tanh(ct)
        dc = dcn + dh * go * (1 - tc*tc)
        dg = torch.cat([dc*gg*gi*(1-gi), dc*cp*gf*(1-gf), dc*gi*(1-gg*gg), dh*tc*go*(1-go)], 1)
        return dg, dc*gf

    def lstm_backward(self, w_hh, act, c, seed, lengths=None):
        w_hh = w_hh.detach()
        N, T, H = c.shape
        dg = torch.zeros_like(act); carry = torch.zeros(N, H)
        ln = torch.full((N,), T) if lengths is None else lengths.long()
        for t in range(T-1, -1, -1):
            valid = (t < ln)[:, None]; has_next = (t+1 < ln)[:, None]
            rec = dg[:, t+1] @ w_hh if t+1 < T else torch.zeros(N, H)
            rec = torch.where(has_next, rec, torch.zeros_like(rec))
            d, cr = self.cell_bwd(act, c, t, seed[:, t] + rec, torch.where(has_next, carry, torch.zeros_like(carry)))
            dg[:, t] = torch.where(valid, d, torch.zeros_like(d)); carry = torch.where(valid, cr, torch.zeros_like(cr))
        return dg

    def attention_backward(self, w_cat, w_query, v, w_loc_dense, w_loc_conv, memory, align, tanh_s, act_a, c_a, base_ctx, base_ah):
        w_cat, w_query, v, w_loc_dense, w_loc_conv = [t.detach() for t in (w_cat, w_query, v, w_loc_dense, w_loc_conv)]
        B, T, Tin = align.shape; A = c_a.shape[2]; E = memory.shape[2]; AD = tanh_s.shape[3]
        NFIL, _, KSZ = w_loc_conv.shape; pad = (KSZ-1)//2
        dgA = torch.zeros(B, T, 4*A); dCTX = torch.zeros(B, T, E); dS = torch.zeros(B, T, Tin, AD); dE = torch.zeros(B, T, Tin)
        gprev = torch.zeros(B, Tin); gcum = torch.zeros(B, Tin); dc = torch.zeros(B, A)
        for t in range(T-1, -1, -1):
            rec = dgA[:, t+1] @ w_cat if t+1 < T else torch.zeros(B, E+A)
            dctx = base_ctx[:, t] + rec[:, :E]; dah = base_ah[:, t] + rec[:, E:]
            dCTX[:, t] = dctx
            dw = torch.einsum("bje,be->bj", memory, dctx) + gcum + gprev
            w = align[:, t]
            de = w * (dw - (w*dw).sum(1, keepdim=True)); dE[:, t] = de
            ds = de[:, :, None] * v[None, None, :] * (1 - tanh_s[:, t]**2); dS[:, t] = ds
            dq = ds.sum(1)
            if t > 0:
                dfeat = ds @ w_loc_dense     # [B,Tin,NFIL]
                din = torch.zeros(B, 2, Tin)
                for c in range(2):
                    for i in range(Tin):
                        s = 0
                        for k in range(KSZ):
                            jj = i - k + pad
                            if 0 <= jj < Tin:
                                s = s + (dfeat[:, jj, :] * w_loc_conv[:, c, k][None]).sum(1)
                        din[:, c, i] = s
                gprev = din[:, 0]; gcum = gcum + din[:, 1]
            dh = dah + dq @ w_query
            d, dc = EmuRec.cell_bwd(act_a, c_a, t, dh, dc if t+1 < T else torch.zeros_like(dc))
            dgA[:, t] = d
        return dgA, dCTX, dS, dE


def torch_forward(model, ppg, lens, tgt, enc_m, dec_m):
    """-> memory, mel, gate, align, ah, dh (all frames), fp64, no grad"""
    hp = model._hp
    with torch.no_grad():
        x = tg.encoder_front(model, ppg, enc_m)
        B, Tin, E = x.shape; H = E // 2
        lstm = model.encoder.lstm
        memory = torch.zeros(B, Tin, E)
        for b in range(B):
            L = int(lens[b])
            for k, sfx in enumerate(("", "_reverse")):
                h = torch.zeros(H); c = torch.zeros(H)
                order = range(L) if k == 0 else range(L-1, -1, -1)
                for t in order:
                    g = getattr(lstm, "weight_ih_l0"+sfx) @ x[b, t] + getattr(lstm, "weight_hh_l0"+sfx) @ h + getattr(lstm, "bias_ih_l0"+sfx) + getattr(lstm, "bias_hh_l0"+sfx)
                    i, f, gg, o = torch.sigmoid(g[:H]), torch.sigmoid(g[H:2*H]), torch.tanh(g[2*H:3*H]), torch.sigmoid(g[3*H:])
                    c = f*c + i*gg; h = o*torch.tanh(c)
                    memory[b, t, k*H:(k+1)*H] = h
        d = model.decoder; att = d.attention_layer
        T = tgt.shape[2]
        x0 = tg.shift(tgt.transpose(1, 2))
        p = tg.prenet(d.prenet.layers, x0, [dec_m[0].transpose(1, 2), dec_m[1].transpose(1, 2)])
        pm = memory @ att.memory_layer.linear_layer.weight.t()
        A, D = d.attention_rnn_dim, d.decoder_rnn_dim
        ah = torch.zeros(B, A); ac = torch.zeros(B, A); dh = torch.zeros(B, D); dc = torch.zeros(B, D)
        w = torch.zeros(B, Tin); cum = torch.zeros(B, Tin); ctx = torch.zeros(B, E)
        AH, DH, AL, OUT = [], [], [], []
        W = hp["attention_window_size"]
        for t in range(T):
            ah, ac = d.attention_rnn(torch.cat([p[:, t], ctx], 1), (ah, ac))
            feat = F.conv1d(torch.stack([w, cum], 1), att.location_layer.location_conv.conv.weight, padding=15)
            loc = feat.transpose(1, 2) @ att.location_layer.location_dense.linear_layer.weight.t()
            e = torch.tanh((ah @ att.query_layer.linear_layer.weight.t())[:, None] + loc + pm) @ att.v.linear_layer.weight.reshape(-1)
            for b in range(B):
                L = int(lens[b])
                if W is not None:
                    lo, hi = min(max(0, t - W), L - 1), min(t + W, L - 1)
                else:
                    lo, hi = 0, L - 1
                m = torch.ones(Tin, dtype=torch.bool); m[lo:hi+1] = False
                e[b, m] = -float("inf")
            w = torch.softmax(e, 1); ctx = torch.einsum("bj,bje->be", w, memory); cum = cum + w
            dh, dc = d.decoder_rnn(torch.cat([ah, ctx], 1), (dh, dc))
            o = torch.cat([dh, ctx], 1)
            OUT.append(torch.cat([F.linear(o, d.linear_projection.linear_layer.weight, d.linear_projection.linear_layer.bias), F.linear(o, d.gate_layer.linear_layer.weight, d.gate_layer.linear_layer.bias)], 1))
            AH.append(ah); DH.append(dh); AL.append(w)
        OUT = torch.stack(OUT, 1)
        return memory, OUT[:, :, :-1].transpose(1, 2).contiguous(), OUT[:, :, -1].contiguous(), torch.stack(AL, 1), torch.stack(AH, 1), torch.stack(DH, 1)
